"""The scenarios of the reference's tests/transforms/nonlinearities_test.py for the elementwise nonlinearities, restated against
the drop-in classes on the device (in the manner of tests/test_gpu_reference_suite.py): same scenarios, sizes and tolerances,
cited by file:line.  (Its piecewise-CDF classes, :33-91, are restated in tests/test_gpu_cdf_shared.py: `test_raises_domain_exception`
and `test_reference_scenarios`, for all four classes.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def good(t, shape=None):
    """transform_test.py's assert_tensor_is_good: a tensor of the shape, no NaN, no inf."""
    assert isinstance(t, torch.Tensor) and not torch.isnan(t).any() and not torch.isinf(t).any()
    if shape is not None:
        assert list(t.shape) == list(shape)


def transforms():
    """nonlinearities_test.py:114-122, :133-141, :152-160"""
    from nflows_amd.transforms import (CompositeCDFTransform, Exp, IdentityTransform, LeakyReLU, Logit, LogTanh, Sigmoid,
                                       Tanh)
    return [t.to(DEV) for t in (Exp(), Tanh(), LogTanh(), LeakyReLU(), Sigmoid(), Logit(),
                                CompositeCDFTransform(Sigmoid(), IdentityTransform()))]


def unit_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    # (torch.rand draws from [0, 1): an exact 0 is outside Exp's inverse domain in the reference as well; the seed has none)
    x = torch.rand(10, 5, 10, 15, generator=gen)
    assert float(x.min()) > 0
    return x.to(DEV)


def test_exp_raises_domain_exception():
    """nonlinearities_test.py:13-20"""
    from nflows_amd.transforms import Exp, InputOutsideDomain
    t = Exp().to(DEV)
    for value in (-1.0, 0.0):
        with pytest.raises(InputOutsideDomain):
            t.inverse(torch.full([2, 3, 4], value, device=DEV))


def test_tanh_raises_domain_exception():
    """nonlinearities_test.py:23-30"""
    from nflows_amd.transforms import InputOutsideDomain, Tanh
    t = Tanh().to(DEV)
    for value in (-2.0, -1.0, 1.0, 2.0):
        with pytest.raises(InputOutsideDomain):
            t.inverse(torch.full([2, 3, 4], value, device=DEV))


def test_logit_forward_zero_and_one():
    """nonlinearities_test.py:94-106: exact zeros and ones are inside the domain and give finite results (the clamp)"""
    from nflows_amd.transforms import Logit
    inputs = torch.cat([torch.zeros(5, 5, 10, 15), torch.ones(5, 5, 10, 15)]).to(DEV)
    outputs, logabsdet = Logit().to(DEV)(inputs)
    good(outputs)
    good(logabsdet)


def test_forward():
    """nonlinearities_test.py:110-127"""
    inputs = unit_inputs(1)
    for t in transforms():
        outputs, logabsdet = t(inputs)
        good(outputs, [10, 5, 10, 15])
        good(logabsdet, [10])


def test_inverse():
    """nonlinearities_test.py:129-146"""
    inputs = unit_inputs(2)
    for t in transforms():
        outputs, logabsdet = t.inverse(inputs)
        good(outputs, [10, 5, 10, 15])
        good(logabsdet, [10])


def test_forward_inverse_are_consistent():
    """nonlinearities_test.py:148-164 with transform_test.py's assert_forward_inverse_are_consistent at eps = 1e-3"""
    inputs = unit_inputs(3)
    eps = 1e-3
    for t in transforms():
        outputs, logabsdet = t(inputs)
        back, logabsdet_inv = t.inverse(outputs)
        good(outputs)
        good(back)
        assert float((back - inputs).abs().max()) <= eps, type(t).__name__
        assert float((logabsdet + logabsdet_inv).abs().max()) <= eps, type(t).__name__
