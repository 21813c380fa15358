from .made import MADE, MixtureOfGaussiansMADE  # noqa: F401
