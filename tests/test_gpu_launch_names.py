"""The launch step on the device, at the smallest sizes that reach C: three entries of three libraries through their public wrappers, and
the same launches again with one tensor of the neighbouring dtype -- refused in Python, by the parameter's name, before C is reached."""
import numpy as np
import pytest
import torch

from onepose_st_amd import pnp_device, pose_eval, track_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _launches_of(mod, monkeypatch, run):
    """``run()`` with ``mod.launch`` recorded -> (what ``run`` returned, [(entry, named, stream), ...]); the real launches happen"""
    seen, real = [], mod.launch
    monkeypatch.setattr(mod, "launch", lambda entry, named, stream=None: seen.append((entry, dict(named), stream)) or real(entry, named, stream))
    out = run()
    monkeypatch.setattr(mod, "launch", real)
    return out, seen


def _refused(mod, monkeypatch, entry, named, name, dtype):
    """the launch with ``named[name]`` replaced by a tensor like it of ``dtype``: a ``TypeError`` naming entry and parameter, nothing called"""
    entered = []
    monkeypatch.setattr(mod, "call", lambda *args: entered.append(args))
    wrong = torch.zeros(named[name].shape, dtype=dtype, device=DEV)
    with pytest.raises(TypeError) as e:
        mod.launch(entry, dict(named, **{name: wrong}))
    assert f"{entry}, {name}: expected {named[name].dtype}, got {dtype}" in str(e.value)
    assert entered == []
    monkeypatch.undo()


def test_long_long_pointer_oppnpd_ranges(monkeypatch):
    b_ids = torch.zeros(4, dtype=torch.int64, device=DEV)
    count = torch.tensor([3], dtype=torch.int32, device=DEV)
    ranges, seen = _launches_of(pnp_device, monkeypatch, lambda: pnp_device.stages.ranges(b_ids, count, 4, 1))
    assert ranges.tolist() == [[0, 3]]
    (entry, named, _), = seen
    assert entry == "oppnpd_ranges" and named["b_ids"] is b_ids and named["count"] is count
    _refused(pnp_device, monkeypatch, entry, named, "b_ids", torch.int32)          # int32 for long long*
    _refused(pnp_device, monkeypatch, entry, named, "count", torch.int64)          # int64 for int*
    _refused(pnp_device, monkeypatch, entry, named, "ranges", torch.int64)


def test_int_pointer_opevl_errors(monkeypatch):
    pose = torch.eye(4, dtype=torch.float64, device=DEV)[None, :3].contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    errs, seen = _launches_of(pose_eval, monkeypatch, lambda: pose_eval.pose_errors(pose, pose.clone(), status=status))
    assert errs.t_err.tolist() == [0.0] and errs.flags.dtype == torch.int32
    (entry, named, _), = seen
    assert entry == "opevl_errors" and named["status"] is status
    _refused(pose_eval, monkeypatch, entry, named, "status", torch.int64)          # int64 for int*
    _refused(pose_eval, monkeypatch, entry, named, "flags", torch.int64)
    _refused(pose_eval, monkeypatch, entry, named, "pose_pred", torch.float32)     # float32 for double*


def test_double_pointer_optrk_box_set(monkeypatch):
    K = torch.tensor([[500.0, 0, 64], [0, 500.0, 48], [0, 0, 1]], dtype=torch.float64, device=DEV)
    st, seen = _launches_of(track_device, monkeypatch, lambda: track_device.set_box([8, 4, 72, 68], K, crop_size=32))
    box, flag, K_crop, trans = st.to_host()
    assert box.tolist() == [8, 4, 72, 68] and np.isfinite(K_crop).all() and np.isfinite(trans).all()
    (entry, named, _), = seen
    assert entry == "optrk_box_set" and named["K"].dtype == torch.float64
    _refused(track_device, monkeypatch, entry, named, "K", torch.float32)          # float32 for double*
    _refused(track_device, monkeypatch, entry, named, "K_crop", torch.float32)
    _refused(track_device, monkeypatch, entry, named, "box", torch.int64)          # int64 for int*
