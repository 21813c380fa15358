from . import functional, nde, nets
