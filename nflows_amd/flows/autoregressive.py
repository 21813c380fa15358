"""Masked autoregressive flow (API of nflows/flows/autoregressive.py)."""
from torch.nn import functional as F

from ..distributions.normal import StandardNormal
from ..transforms.autoregressive import MaskedAffineAutoregressiveTransform
from ..transforms.base import CompositeTransform
from ..transforms.normalization import BatchNorm
from ..transforms.permutations import RandomPermutation, ReversePermutation
from .base import Flow


class MaskedAutoregressiveFlow(Flow):
    """`num_layers` times [permutation (reversal, or random with `use_random_permutations`), affine MADE layer, and with
    `batch_norm_between_layers` a `BatchNorm`] on a standard normal base (Papamakarios et al., NeurIPS 2017).  Modules
    are created in the reference's order: the same seed gives the same weights and permutations."""

    def __init__(self, features, hidden_features, num_layers, num_blocks_per_layer, use_residual_blocks=True,
                 use_random_masks=False, use_random_permutations=False, activation=F.relu, dropout_probability=0.0,
                 batch_norm_within_layers=False, batch_norm_between_layers=False):
        permutation = RandomPermutation if use_random_permutations else ReversePermutation
        layers = []
        for _ in range(num_layers):
            layers.append(permutation(features))
            layers.append(MaskedAffineAutoregressiveTransform(
                features=features, hidden_features=hidden_features, num_blocks=num_blocks_per_layer,
                use_residual_blocks=use_residual_blocks, random_mask=use_random_masks, activation=activation,
                dropout_probability=dropout_probability, use_batch_norm=batch_norm_within_layers))
            if batch_norm_between_layers:
                layers.append(BatchNorm(features))
        super().__init__(transform=CompositeTransform(layers), distribution=StandardNormal([features]))
