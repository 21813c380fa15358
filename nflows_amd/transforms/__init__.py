from .base import (CompositeTransform, InputOutsideDomain, InverseNotAvailable, InverseTransform,
                   MultiscaleCompositeTransform, Transform)
from .standard import AffineScalarTransform, AffineTransform, IdentityTransform, PointwiseAffineTransform
from .coupling import (AdditiveCouplingTransform, AffineCouplingTransform, CouplingTransform,
                       PiecewiseCubicCouplingTransform, PiecewiseLinearCouplingTransform,
                       PiecewiseQuadraticCouplingTransform,
                       PiecewiseRationalQuadraticCouplingTransform)
from .permutations import Permutation, RandomPermutation, ReversePermutation
from .linear import Linear, NaiveLinear
from .lu import LULinear
from .orthogonal import HouseholderSequence
from .svd import SVDLinear
from .qr import QRLinear
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
