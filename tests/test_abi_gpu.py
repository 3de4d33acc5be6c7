"""GPU: the one launch helper of the C-ABI binding (`_lib.call`) -- stream appended, error code -> RuntimeError."""
import pytest

pytestmark = pytest.mark.gpu


def test_call_raises_with_entry_point_and_last_error(dev):
    """Null pointers and B = 0 are refused by the library's host-side argument check (RFN_EINVAL): nothing is launched."""
    from refign_amd import _lib
    with pytest.raises(RuntimeError) as e:
        _lib.call("rfn_corr_fwd_f32", dev, None, None, None, 0, 1, 4, 4, 1, 1, 9, 9, 0, 0, 1, 1, 1, 1, 1, 1)
    last = _lib.load_library().rfn_last_error().decode()
    assert last and last in str(e.value)
    assert "rfn_corr_fwd_f32" in str(e.value).split(last)[0] and "code -1" in str(e.value)
