"""`vatl_sgd_step_multi` (csrc/optim.hip): one launch per (parameter group, step count) behind ``active_learning.optim.SGD``, the
per-tensor kernel's bits in both of its forms (step 1: buf = g; later steps: body / tail arithmetic split), and the recorded bits of
tests/golden/optim_bits.npz."""
import numpy as np
import pytest
import torch

from tests import optim_cases
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _tensors(vh, seed):
    """Parameters of 1 and 3 elements, around the multi kernel's block size E, over two blocks, and a contiguous view whose base is
    only 4-byte aligned."""
    E = int(vh.lib().vatl_adamw_multi_block_elems())
    r = np.random.RandomState(seed)
    sizes = [1, 3, E - 1, E, E + 1, 2 * E + 3]
    ps = [torch.nn.Parameter(to_dev(r.standard_normal(n).astype(np.float32))) for n in sizes]
    holder = to_dev(r.standard_normal(1100).astype(np.float32))
    view = torch.nn.Parameter(holder[1:1 + 1003])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return r, ps + [view]


def _grads(r, ps):
    """Fresh gradients; the one of the 4-byte-aligned parameter is itself a view at another 4-byte-aligned base."""
    gs = [to_dev(r.standard_normal(tuple(p.shape)).astype(np.float32)) for p in ps[:-1]]
    g = r.standard_normal(tuple(ps[-1].shape)).astype(np.float32)
    gs.append(to_dev(np.concatenate([np.zeros(3, np.float32), g]))[3:])
    return gs


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_sgd_multi_equals_per_tensor_bit_for_bit(vh, wd, monkeypatch):
    """Through optim.SGD against `vatl_sgd_step` tensor by tensor on 16-byte-aligned clones (the per-tensor entry's contract): equal
    bits after 3 steps, so both forms of the update — `buf = g` at step 1, the body / tail split after — ran in the multi kernel.  The
    unaligned view rides the multi launch's scalar path, which must still give elements below 4 * (n / 4) the float4 body's
    arithmetic.  One `vatl_sgd_step_multi` call per optimiser step, no per-tensor call."""
    from active_learning import optim
    calls = {"multi": 0, "single": 0}
    multi, single = optim.SGD._multi, optim.SGD._kernel
    assert multi is not None
    monkeypatch.setattr(optim.SGD, "_multi", staticmethod(lambda *a: (calls.__setitem__("multi", calls["multi"] + 1), multi(*a))[1]))
    monkeypatch.setattr(optim.SGD, "_kernel", staticmethod(lambda *a: (calls.__setitem__("single", calls["single"] + 1), single(*a))[1]))
    r, ps = _tensors(vh, 31)
    skipped = torch.nn.Parameter(to_dev(r.standard_normal(33).astype(np.float32)))       # never gets a gradient
    before = skipped.detach().clone()
    qs = [p.detach().clone() for p in ps]
    bufs = [torch.zeros_like(q) for q in qs]
    opt = optim.SGD(ps + [skipped], lr=2.5e-4, momentum=0.9, weight_decay=wd)
    for step in range(1, 4):
        gs = _grads(r, ps)
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        for q, g, b in zip(qs, gs, bufs):
            vh.sgd_step(q, g.clone(), b, step, 2.5e-4, 0.9, wd)
    for p, q, b in zip(ps, qs, bufs):
        bad = int((p.detach().view(torch.int32) != q.view(torch.int32)).sum())
        print(f"wd {wd} n {p.numel()}: {bad} of {p.numel()} elements differ")
        assert torch.equal(p.detach(), q) and p._version > 0, p.numel()
        assert torch.equal(opt.state[p]["momentum_buffer"], b), p.numel()
    assert torch.equal(skipped.detach(), before) and skipped not in opt.state
    assert calls == {"multi": 3, "single": 0}, calls


def test_a_strided_parameter_takes_the_per_tensor_route(vh, monkeypatch):
    """`_Stepper.step` hands a group to the multi entry only when every parameter is contiguous; a strided slice sends the whole group
    tensor by tensor through `vatl_sgd_step` — the contiguous members with the multi launch's bits, and the strided one to that entry's
    own refusal (it takes flat spans only)."""
    from active_learning import optim
    seen = []
    single = optim.SGD._kernel
    monkeypatch.setattr(optim.SGD, "_multi", staticmethod(lambda *a: seen.append("multi")))
    monkeypatch.setattr(optim.SGD, "_kernel", staticmethod(lambda *a: (seen.append("single"), single(*a))[1]))
    r = np.random.RandomState(37)
    a = torch.nn.Parameter(to_dev(r.standard_normal(1027).astype(np.float32)))
    strided = torch.nn.Parameter(to_dev(r.standard_normal((64, 2)).astype(np.float32))[:, 0])
    assert not strided.is_contiguous()
    q, b = a.detach().clone(), torch.zeros(1027, device=a.device)
    g = to_dev(r.standard_normal(1027).astype(np.float32))
    a.grad, strided.grad = g, torch.zeros(64, device=a.device)
    opt = optim.SGD([a, strided], lr=1e-2, momentum=0.9)
    with pytest.raises(vh.VatlError, match="contiguous"):
        opt.step()
    assert seen == ["single", "single"]
    vh.sgd_step(q, g, b, 1, 1e-2, 0.9, 0.0)
    assert torch.equal(a.detach(), q)


@pytest.mark.parametrize("route", ["multi", "multi_view"])
def test_sgd_multi_writes_the_recorded_bits(vh, route):
    """The `sgd` case of tests/optim_cases.py (1027 elements: 1024 on the float4 body's arithmetic and a tail of 3; 3 steps, so both
    forms) through the multi entry reproduces tests/golden/optim_bits.npz — also from bases that are only 4-byte aligned."""
    golden = np.load(optim_cases.GOLDEN)
    p0, gs = optim_cases.inputs("sgd")

    def place(a):
        if route == "multi":
            return to_dev(a)
        v = to_dev(np.concatenate([np.zeros(1, np.float32), a, np.zeros(3, np.float32)]))[1:1 + a.size]
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    p, buf = place(p0), place(np.zeros_like(p0))
    optim_cases.run(vh, "sgd", p, [place(g) for g in gs], [buf], multi=True)
    for name, t in (("p", p), ("momentum_buffer", buf)):
        got, want = optim_cases.bits(t), golden[f"sgd_{name}"]
        bad = np.flatnonzero(got != want)
        print(f"sgd {route} {name}: {bad.size} of {want.size} elements differ", bad[:8])
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


def test_sgd_multi_rejects_what_the_other_multi_entries_reject(vh):
    p = torch.zeros(8, device="cuda")
    with pytest.raises(vh.VatlError, match="1-based"):
        vh.sgd_step_multi([p], [p.clone()], [p.clone()], 0, 1e-3)
    vh.sgd_step_multi([], [], [], 1, 1e-3)                                                 # nothing to do
    with pytest.raises(vh.VatlError, match="contiguous fp32"):
        vh.sgd_step_multi([p.double()], [p.clone()], [p.clone()], 1, 1e-3)
