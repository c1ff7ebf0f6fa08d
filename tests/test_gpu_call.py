"""_C.call on the device: what one launch hands its entry point (addresses, NULL, the caller's stream on the operands'
device), that it refuses operands on another device before launching, and how it reports the status.  The entry point is
a recording stand-in: nothing is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Recorder:
    def __init__(self, rc=0):
        self.rc, self.args, self.device = rc, None, None

    def __call__(self, *args):
        self.args, self.device = args, torch.cuda.current_device()
        return self.rc


@pytest.fixture
def rec(monkeypatch):
    from splatco_amd import _C
    r = _Recorder()
    monkeypatch.setattr(_C.lib, "scr_copy_probe", r)
    return r


def test_call_passes_addresses_null_scalars_and_the_callers_stream(rec):
    from splatco_amd import _C
    a, b = torch.zeros(4, device="cuda:0"), torch.ones(4, dtype=torch.int32, device="cuda:0")
    arr = _C.host_array((1, 2, 3))
    assert _C.call("scr_copy_probe", 3, a, None, 2.5, arr, b[1:], a.data_ptr() + 8) == 0
    want = (3, a.data_ptr(), None, 2.5, arr, b.data_ptr() + 4, a.data_ptr() + 8)
    assert rec.args[:-1] == want and rec.args[4] is arr
    assert len(rec.args) == len(want) + 1 and rec.args[-1] == torch.cuda.current_stream(a.device).cuda_stream
    s = torch.cuda.Stream(device=a.device)
    with torch.cuda.stream(s):
        _C.call("scr_copy_probe", a)
    assert rec.args == (a.data_ptr(), s.cuda_stream)
    _C.call("scr_copy_probe", 5, device=a.device)          # operands in tables only: the device is named
    assert rec.args == (5, torch.cuda.current_stream(a.device).cuda_stream)


def test_call_refuses_a_cpu_tensor_among_device_tensors(rec):
    from splatco_amd import _C
    a = torch.zeros(4, device="cuda:0")
    with pytest.raises(ValueError) as e:
        _C.call("scr_copy_probe", 4, a, a, torch.zeros(4))
    assert "scr_copy_probe" in str(e.value) and "argument 3" in str(e.value) and "cpu" in str(e.value) and "cuda:0" in str(e.value)
    assert rec.args is None


def test_call_raises_or_returns_the_status(rec):
    from splatco_amd import _C
    a = torch.zeros(4, device="cuda:0")
    rec.rc = 3
    assert _C.call("scr_copy_probe", a, check=False) == 3
    with pytest.raises(RuntimeError, match="^splatco_raster: "):
        _C.call("scr_copy_probe", a)


def test_call_makes_the_operands_device_current(rec):
    """Only observable with a second device: the stand-in sees device 1 current while device 0 is current outside."""
    from splatco_amd import _C
    if torch.cuda.device_count() > 1:
        assert torch.cuda.current_device() == 0
        a = torch.zeros(4, device="cuda:1")
        _C.call("scr_copy_probe", a)
        assert rec.device == 1 and torch.cuda.current_device() == 0
        assert rec.args == (a.data_ptr(), torch.cuda.current_stream(a.device).cuda_stream)
