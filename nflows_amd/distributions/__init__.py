from .base import Distribution, NoMeanException  # noqa: F401
from .discrete import ConditionalIndependentBernoulli  # noqa: F401
from .mixture import MADEMoG  # noqa: F401
from .normal import ConditionalDiagonalNormal, DiagonalNormal, StandardNormal  # noqa: F401
from .uniform import LotkaVolterraOscillating, MG1Uniform  # noqa: F401
