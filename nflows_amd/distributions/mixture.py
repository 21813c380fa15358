"""`MADEMoG` (reference: nflows/distributions/mixture.py): a mixture-of-Gaussians MADE as a `Distribution`.  The density is
`nn.nde.MixtureOfGaussiansMADE.log_prob`: the MADE's forward pass, then one launch of K20 "mog" on a HIP device.
`sample` (and `sample_and_log_prob`, and every Flow with this base) is `MixtureOfGaussiansMADE.sample`: on a HIP device one
launch of K30 on `torch.rand(B, D)` and then `torch.randn(B, D)` from the default generator -- other draws than the host
loop's for a given seed, the same distribution; `NFA_K30=0` gives the host loop (see nn/nde/made.py)."""
from torch.nn import functional as F

from ..nn.nde import MixtureOfGaussiansMADE
from .base import Distribution


class MADEMoG(Distribution):
    def __init__(self, features, hidden_features, context_features, num_blocks=2, num_mixture_components=1,
                 use_residual_blocks=True, random_mask=False, activation=F.relu, dropout_probability=0.0,
                 use_batch_norm=False, custom_initialization=False):
        super().__init__()
        self._made = MixtureOfGaussiansMADE(
            features=features, hidden_features=hidden_features, context_features=context_features, num_blocks=num_blocks,
            num_mixture_components=num_mixture_components, use_residual_blocks=use_residual_blocks, random_mask=random_mask,
            activation=activation, dropout_probability=dropout_probability, use_batch_norm=use_batch_norm,
            custom_initialization=custom_initialization)

    def _log_prob(self, inputs, context=None):
        return self._made.log_prob(inputs, context=context)

    def _sample(self, num_samples, context=None):
        return self._made.sample(num_samples, context=context)
