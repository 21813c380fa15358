from .torchutils import (create_alternating_binary_mask, create_mid_split_binary_mask,
                         create_random_binary_mask, logabsdet, merge_leading_dims, random_orthogonal, repeat_rows,
                         split_leading_dim, sum_except_batch, searchsorted)
from . import typechecks
