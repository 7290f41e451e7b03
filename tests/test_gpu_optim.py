"""The element-wise optimisers (csrc/optim.hip: AdamW, Adam, SGD, RMSprop; per-tensor and one-launch multi-tensor entries): their bits
against tests/golden/optim_bits.npz, the multi entries against the per-tensor ones, and the steps against torch / the numpy oracle."""
import numpy as np
import pytest
import torch

from oracle import scorers
from tests import optim_cases
from tests.gpu_util import record, rel_err, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


@pytest.fixture(scope="module")
def golden_bits():
    return np.load(optim_cases.GOLDEN)


def _view_at_4(a):
    """A contiguous device copy of ``a`` whose base is 4-byte but not 16-byte aligned."""
    holder = to_dev(np.concatenate([np.zeros(1, np.float32), a, np.zeros(3, np.float32)]))
    view = holder[1:1 + a.size]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("kind,route", [(k, "flat") for k in optim_cases.CASES]
                         + [(k, r) for r in ("multi", "multi_view") for k in ("adamw", "adam", "rmsprop")])
def test_bits_are_the_recorded_ones(vh, golden_bits, kind, route):
    """Every route that reaches a kind writes the bits recorded from the commit before csrc/optim.hip existed (tools/make_optim_bits.py,
    per-tensor entries on aligned tensors): the flat entry, the multi entry, and the multi entry on views whose bases are only 4-byte
    aligned — the scalar path throughout, where the first 1024 of the 1027 elements still take the float4 body's arithmetic.

    Against that parent commit's own library (VATL_HIP_LIB) every case passes but adamw-multi_view (518 of the 1027 elements of p differ):
    its adamw_multi_kernel gave every element of an unaligned tensor the TAIL form (mul, then add), not its per-tensor kernel's bits
    (profiles/optim_unify_notes.md)."""
    p0, gs = optim_cases.inputs(kind)
    place = _view_at_4 if route == "multi_view" else to_dev
    names = optim_cases.CASES[kind][1]
    p, bufs = place(p0), [place(np.zeros_like(p0)) for _ in names]
    optim_cases.run(vh, kind, p, [place(g) for g in gs], bufs, multi=route != "flat")
    for name, t in zip(("p",) + names, [p] + bufs):
        got, want = optim_cases.bits(t), golden_bits[f"{kind}_{name}"]
        bad = np.flatnonzero(got != want)
        print(f"{kind} {route} {name}: {bad.size} of {want.size} elements differ", bad[:8])
        assert bad.size == 0, (kind, route, name, bad[:8], got[bad[:8]], want[bad[:8]])


def test_adam_and_sgd_steps(vh):
    """ActiveLearning.py:220-223: the two other optimisers the reference can be configured with."""
    from active_learning.optim import SGD, Adam
    r = np.random.RandomState(5)
    n = 70001
    p0 = r.standard_normal(n).astype(np.float32)
    a, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    b, buf = p0.copy(), np.zeros(n, np.float32)
    da = torch.nn.Parameter(to_dev(p0)); ds = torch.nn.Parameter(to_dev(p0))
    oa, os_ = Adam([da], lr=2.5e-4), SGD([ds], lr=2.5e-4, momentum=0.9, weight_decay=0.0005)
    for step in range(1, 5):
        g = r.standard_normal(n).astype(np.float32)
        da.grad = to_dev(g); ds.grad = to_dev(g)
        oa.step(); os_.step()
        a, m, v = scorers.adam_step(a, g, m, v, step, 2.5e-4)
        b, buf = scorers.sgd_step(b, g, buf, step, 2.5e-4, 0.9, 0.0005)
    record("adam_step", rel=rel_err(da.detach().cpu().numpy(), a)); record("sgd_step", rel=rel_err(ds.detach().cpu().numpy(), b))
    np.testing.assert_allclose(da.detach().cpu().numpy(), a, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(ds.detach().cpu().numpy(), b, rtol=2e-6, atol=1e-7)
    assert da._version > 0 and ds._version > 0           # plan caches key on the version counter


def _optimiser_tensors(vh, seed):
    """Parameters around the multi kernel's block size, a conv weight, and a view whose base is only 4-byte aligned."""
    E = int(vh.lib().vatl_adamw_multi_block_elems())
    r = np.random.RandomState(seed)
    shapes = [(1,), (17,), (E - 1,), (E,), (E + 1,), (2 * E + 3,), (64, 32, 3, 3)]
    ps = [torch.nn.Parameter(to_dev(r.standard_normal(s).astype(np.float32))) for s in shapes]
    buf = to_dev(r.standard_normal(1100).astype(np.float32))
    view = torch.nn.Parameter(buf[1:1 + 1001])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ps.append(view)
    skipped = torch.nn.Parameter(to_dev(r.standard_normal(33).astype(np.float32)))       # never gets a gradient
    return E, r, ps, skipped


def _grads_like(r, ps, misalign):
    """Fresh gradients; the one of the 4-byte-aligned parameter is itself a view at a 4-byte-aligned base."""
    gs = []
    for k, p in enumerate(ps):
        g = r.standard_normal(tuple(p.shape)).astype(np.float32)
        if k == misalign:
            holder = to_dev(np.concatenate([np.zeros(3, np.float32), g.reshape(-1)]))
            gs.append(holder[3:].view(p.shape))
        else:
            gs.append(to_dev(g))
    return gs


def test_multi_tensor_adamw_equals_per_tensor(vh):
    """One launch per parameter group (`vatl_adamw_step_multi`) against the per-tensor kernel: same bits, odd sizes and
    unaligned tails included; the optimizer class uses it and bumps every parameter's version counter."""
    from active_learning.optim import AdamW
    r = np.random.RandomState(17)
    sizes = [(64,), (17,), (256, 64, 3, 3), (1001,), (5, 7), (2048, 512, 1, 1)]
    ps = [torch.nn.Parameter(to_dev(r.standard_normal(s).astype(np.float32))) for s in sizes]
    _, r2, extra, _ = _optimiser_tensors(vh, 19)          # sizes around the block size and a view at a 4-byte-aligned base
    ps += extra
    qs = [p.detach().clone() for p in ps]                 # (clones are 16-byte aligned: the per-tensor kernel's contract)
    ms, vs = [torch.zeros_like(q) for q in qs], [torch.zeros_like(q) for q in qs]
    opt = AdamW([{"params": ps[:2], "lr": 2.5e-3}, {"params": ps[2:], "lr": 2.5e-4}], weight_decay=0.7)
    for step in range(1, 4):
        gs = [to_dev(r.standard_normal(s).astype(np.float32)) for s in sizes] + _grads_like(r2, extra, misalign=len(extra) - 1)
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        for k, (q, g, m, v) in enumerate(zip(qs, gs, ms, vs)):
            vh.adamw_step(q, g.clone(), m, v, step, 2.5e-3 if k < 2 else 2.5e-4, 0.7)
    for p, q, m, v in zip(ps, qs, ms, vs):
        assert torch.equal(p.detach(), q) and p._version > 0, tuple(p.shape)
        assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v), tuple(p.shape)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_multi_equals_per_tensor_bit_for_bit(vh, wd):
    """`vatl_adam_step_multi` behind optim.Adam against `vatl_adam_step` tensor by tensor: the same bits after 3 steps, for sizes around
    the block size, an unaligned base and a parameter without gradient; every stepped parameter's version counter moved."""
    from active_learning.optim import Adam
    E, r, ps, skipped = _optimiser_tensors(vh, 23)
    qs = [p.detach().clone() for p in ps]                                      # (clones are 16-byte aligned: the per-tensor kernel's contract)
    ms, vs = [torch.zeros_like(q) for q in qs], [torch.zeros_like(q) for q in qs]
    before = skipped.detach().clone()
    opt = Adam(ps + [skipped], lr=1e-3, weight_decay=wd)
    assert Adam._multi is not None
    for step in range(1, 4):
        gs = _grads_like(r, ps, misalign=len(ps) - 1)
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        for q, g, m, v in zip(qs, gs, ms, vs):
            vh.adam_step(q, g.clone(), m, v, step, 1e-3, wd)
    for p, q, m, v in zip(ps, qs, ms, vs):
        assert torch.equal(p.detach(), q) and p._version > 0, tuple(p.shape)
        assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
    assert torch.equal(skipped.detach(), before) and skipped not in opt.state


def _rmsprop_f64(p, g, sq, lr, alpha, eps, wd):
    g = g + wd * p
    sq = alpha * sq + (1 - alpha) * g * g
    return p - lr * g / (np.sqrt(sq) + eps), sq


def test_rmsprop_multi_equals_per_tensor_and_torch(vh):
    """`vatl_rmsprop_step_multi` behind optim.RMSprop: the same bits as `vatl_rmsprop_step` per tensor, and 4 steps against
    torch.optim.RMSprop on the CPU (lr 1e-3, weight_decay 5e-4) at the Adam test's bar, rtol 2e-5 / atol 1e-6.  The distance of
    torch's own fp32 result from a float64 restatement of the same steps is recorded beside ours (measured: 3.3e-7 both)."""
    from active_learning.optim import RMSprop
    E, r, ps, skipped = _optimiser_tensors(vh, 29)
    lr, wd = 1e-3, 5e-4
    qs = [p.detach().clone() for p in ps]
    sqs = [torch.zeros_like(q) for q in qs]
    ts = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    f64 = [(p.detach().cpu().double().numpy(), np.zeros(tuple(p.shape))) for p in ps]
    opt, topt = RMSprop(ps + [skipped], lr=lr, weight_decay=wd), torch.optim.RMSprop(ts, lr=lr, weight_decay=wd)
    for step in range(1, 5):
        gs = _grads_like(r, ps, misalign=len(ps) - 1)
        for p, t, g in zip(ps, ts, gs):
            p.grad, t.grad = g, g.cpu().clone()
        opt.step(); topt.step()
        for q, g, sq in zip(qs, gs, sqs):
            vh.rmsprop_step(q, g, sq, lr, weight_decay=wd)
        f64 = [_rmsprop_f64(p64, g.cpu().double().numpy(), s64, lr, 0.99, 1e-8, wd) for (p64, s64), g in zip(f64, gs)]
    ours_worst = torch_worst = 0.0
    for p, q, sq, t, (p64, _) in zip(ps, qs, sqs, ts, f64):
        assert torch.equal(p.detach(), q) and torch.equal(opt.state[p]["square_avg"], sq) and p._version > 0, tuple(p.shape)
        got, want = p.detach().cpu().numpy(), t.detach().numpy()
        ours_worst = max(ours_worst, float(np.abs(got - p64).max()))
        torch_worst = max(torch_worst, float(np.abs(want - p64).max()))
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-6)
    print(f"rmsprop after 4 steps, max abs distance from float64: ours {ours_worst:.3e}, torch fp32 {torch_worst:.3e}")
    record("rmsprop_step", ours_vs_f64=ours_worst, torch_fp32_vs_f64=torch_worst)
    assert skipped not in opt.state
