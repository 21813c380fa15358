"""Real NVP on feature vectors (API of nflows/flows/realnvp.py)."""
import torch
from torch.nn import functional as F

from ..distributions.normal import StandardNormal
from ..nn.nets import ResidualNet
from ..transforms.base import CompositeTransform
from ..transforms.coupling import AdditiveCouplingTransform, AffineCouplingTransform
from ..transforms.normalization import BatchNorm
from .base import Flow


class SimpleRealNVP(Flow):
    """`num_layers` affine (or, with `use_volume_preserving`, additive) couplings on a +-1 mask that flips from layer to
    layer, ResidualNet conditioners, no permutations and no multi-scale splitting (Dinh et al., ICLR 2017), a standard
    normal base.  `batch_norm_between_layers` puts a `BatchNorm` behind every coupling: each coupling then is a launch of
    its own, and each BatchNorm is one K17 launch (plus the statistics in training mode).  Without it the couplings form
    one run of the whole-layer kernel K11.  Modules are created in the reference's order: the same seed gives the same
    weights."""

    def __init__(self, features, hidden_features, num_layers, num_blocks_per_layer, use_volume_preserving=False,
                 activation=F.relu, dropout_probability=0.0, batch_norm_within_layers=False,
                 batch_norm_between_layers=False):
        coupling = AdditiveCouplingTransform if use_volume_preserving else AffineCouplingTransform

        def conditioner(in_features, out_features):
            return ResidualNet(in_features, out_features, hidden_features=hidden_features,
                               num_blocks=num_blocks_per_layer, activation=activation,
                               dropout_probability=dropout_probability, use_batch_norm=batch_norm_within_layers)

        mask = torch.ones(features)
        mask[::2] = -1
        layers = []
        for _ in range(num_layers):
            layers.append(coupling(mask=mask, transform_net_create_fn=conditioner))
            mask = -mask
            if batch_norm_between_layers:
                layers.append(BatchNorm(features=features))
        super().__init__(transform=CompositeTransform(layers), distribution=StandardNormal([features]))
