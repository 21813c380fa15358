from .base import (CompositeTransform, InputOutsideDomain, InverseNotAvailable, InverseTransform,
                   MultiscaleCompositeTransform, Transform)
from .standard import AffineScalarTransform, AffineTransform, IdentityTransform, PointwiseAffineTransform
from .coupling import (AdditiveCouplingTransform, AffineCouplingTransform, CouplingTransform,
                       PiecewiseCubicCouplingTransform, PiecewiseLinearCouplingTransform,
                       PiecewiseQuadraticCouplingTransform,
                       PiecewiseRationalQuadraticCouplingTransform)
from .permutations import Permutation, RandomPermutation, ReversePermutation
from .linear import Linear
from .lu import LULinear
from .conv import OneByOneConvolution
from .reshape import SqueezeTransform
from .normalization import ActNorm, BatchNorm
from . import splines
from .autoregressive import (AutoregressiveTransform, MaskedAffineAutoregressiveTransform,
                             MaskedPiecewiseCubicAutoregressiveTransform,
                             MaskedPiecewiseLinearAutoregressiveTransform,
                             MaskedPiecewiseQuadraticAutoregressiveTransform,
                             MaskedPiecewiseRationalQuadraticAutoregressiveTransform)
from .made import MADE
from .nonlinearities import (CauchyCDF, CauchyCDFInverse, CompositeCDFTransform, Exp, GatedLinearUnit, LeakyReLU, Logit,
                            LogTanh, PiecewiseCubicCDF, PiecewiseLinearCDF, PiecewiseQuadraticCDF,
                            PiecewiseRationalQuadraticCDF, Sigmoid, Tanh)
