"""The fp32-storage interface without a device: the three symbols, the kernel mapping (sglm_pass_kernel_for
flag 4) and the refusals that need no data."""
import numpy as np
import pytest

from sparkglm_amd import Engine
from sparkglm_amd import _lib as L

SYMBOLS = ("sglm_set_data_f32", "sglm_store_f32", "sglm_get_storage")


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbols_are_exported(name):
    assert name in L.EXPORTS and hasattr(L.load(), name)


@pytest.mark.parametrize("p", [1, 16, 17, 32, 33, 48, 64])
def test_kernel_mapping(p):
    kind, name = L.pass_kernel_for(100_000, p, f32=True)
    assert (kind, name) == ("narrow-f32", f"irls_narrow_f32_kernel<{(p + 15) // 16},binomial,logit>")


def test_kernel_mapping_refuses_wider_designs():
    with pytest.raises(L.IllegalArgumentException, match="p <= 64"):
        L.pass_kernel_for(100_000, 65, f32=True)


def test_null_handle():
    lib = L.load()
    assert lib.sglm_store_f32(None) == L.SGLM_EINVAL
    assert lib.sglm_set_data_f32(None, None, 1, 1, 1, None, None, None, None) == L.SGLM_EINVAL


def test_unknown_storage_is_refused_before_the_library_is_called():
    e = Engine.__new__(Engine)  # no handle, no device: the check comes first
    with pytest.raises(L.IllegalArgumentException, match="storage"):
        e.set_data(np.ones((4, 2)), np.ones(4), storage="f16")
    with pytest.raises(L.IllegalArgumentException, match="storage"):
        e.synth(0, 0, 100, 4, 1, storage="f16")  # before the resident data is replaced
