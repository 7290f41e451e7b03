"""The one-launch re-pack of the 16-bit filters (csrc/pack_h16.hip: vatl_pack_weights_h16_multi behind vatl_hip.PackPlanH16) against the
per-tensor packers it replaces, byte for byte, and the plan's life cycle on the bf16 trainer of a SimplePose-R50."""
import pytest
import torch

from oracle import synth
from tests import train_h16_cases as TC
from tests.gpu_util import dev, to_dev

pytestmark = pytest.mark.gpu

GUARD, GUARD_BITS, JUNK_BITS = 64, 0x5A5A, 0x1234      # elements on either side of a destination; what they hold; what the destination holds before


@pytest.fixture(scope="module")
def vh():
    import vatl_hip
    vatl_hip.lib()
    return vatl_hip


def _filters():
    """Every filter shape of tests/train_h16_cases.py once -> [(name, source shape, stride, pad, transposed)]."""
    out, seen = [], set()
    for cases in (TC.WGRAD_CASES, TC.DGRAD_CASES):
        for name, case in cases.items():
            _, cin, cout, _, _, r, stride, pad = case[:8]
            if (cout, cin, r, stride, pad) not in seen:
                seen.add((cout, cin, r, stride, pad))
                out.append((name, (cout, cin, r, r), stride, pad, False))
    for name, case in list(TC.WGRAD_DECONV_CASES.items()) + [("dgrad_deconv", TC.DGRAD_DECONV_CASE)]:
        _, cin, cout = case[:3]
        if ("deconv", cin, cout) not in seen:
            seen.add(("deconv", cin, cout))
            out.append((name, (cin, cout, 4, 4), 2, 1, True))
    return out


def _per_tensor(vh, kind, w, stride, pad, dtype):
    if kind == vh.PACK_H16_CONV:
        return vh.pack_conv_weight_h16(w, dtype)
    if kind == vh.PACK_H16_DECONV:
        return vh.pack_deconv_weight_h16(w, dtype)
    return vh.pack_conv_weight_dgrad_h16(w, stride, pad, dtype)


def _jobs(vh, dtype, seed=0):
    """[(name, kind, source, stride, pad, the per-tensor packer's output as int16)]: each shape as a forward job and a data-gradient job
    (a transposed conv's data gradient is the conv forward pack of its (Cin,Cout,4,4) weight)."""
    gen = torch.Generator().manual_seed(seed)
    jobs = []
    for name, shape, stride, pad, transposed in _filters():
        w = torch.randn(shape, generator=gen).to(dev())
        kinds = (vh.PACK_H16_DECONV, vh.PACK_H16_CONV) if transposed else (vh.PACK_H16_CONV, vh.PACK_H16_DGRAD)
        for kind in kinds:
            jobs.append((f"{name}/{kind}", kind, w, stride, pad, _per_tensor(vh, kind, w, stride, pad, dtype).view(torch.int16).reshape(-1).clone()))
    return jobs


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def table(request, vh):
    return request.param, _jobs(vh, request.param)


def _guarded(n, dtype):
    """A destination of n elements between two guard bands -> (whole buffer as int16, the destination as ``dtype``)."""
    buf = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int16, device=dev())
    buf[GUARD:GUARD + n] = JUNK_BITS
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _plan_of(vh, dtype, jobs):
    plan = vh.PackPlanH16(dtype)
    plan.begin()                                                       # nothing recorded yet: no launch
    held = []
    for name, kind, w, stride, pad, want in jobs:
        buf, dst = _guarded(want.numel(), dtype)
        plan.record(name, w, dst, kind, stride, pad)
        held.append((name, buf, dst, want))
    plan.seal()
    return plan, held


def _check(held):
    for name, buf, dst, want in held:
        assert torch.equal(dst.view(torch.int16), want), name
        assert bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[-GUARD:] == GUARD_BITS).all()), name


def test_the_case_table_covers_what_a_packer_can_get_wrong(vh):
    shapes = {(s, st, p) for _, s, st, p, _ in _filters()}
    for need in (((64, 3, 7, 7), 2, 3), ((24, 16, 3, 3), 1, 1), ((24, 8, 3, 3), 2, 1), ((32, 8, 1, 1), 2, 0), ((16, 512, 3, 3), 1, 1), ((17, 16, 1, 1), 1, 0),
                 ((8, 8, 4, 4), 2, 1)):
        assert need in shapes, need
    assert vh.PackPlanH16.elements(vh.PACK_H16_CONV, (16, 512, 3, 3)) > 64 * 1024          # a job of many blocks


@pytest.mark.parametrize("order", ["forward", "reversed", "single"])
def test_one_launch_writes_the_per_tensor_bytes(vh, table, order):
    dtype, jobs = table
    jobs = {"forward": jobs, "reversed": jobs[::-1], "single": [j for j in jobs if j[2].shape[1] == 512][:1]}[order]
    plan, held = _plan_of(vh, dtype, jobs)
    assert plan.ready and len(plan.jobs) == len(jobs) and (order != "single" or len(jobs) == 1)
    assert plan.total_blocks == sum((want.numel() + 1023) // 1024 for *_, want in jobs)
    for name, buf, dst, want in held:                                  # nothing has been launched yet
        assert bool((dst.view(torch.int16) == JUNK_BITS).all()), name
    plan.begin()                                                       # ONE launch
    torch.cuda.synchronize()
    _check(held)
    for (name, kind, w, *_), (_, _, dst, _) in zip(jobs, held):
        assert plan.lookup(name, w) is dst
    assert not plan.stale


def test_second_begin_refreshes_after_in_place_changes(vh):
    dtype = torch.bfloat16
    jobs = _jobs(vh, dtype, seed=1)
    plan, held = _plan_of(vh, dtype, jobs)
    plan.begin()
    for _, _, w, *_ in jobs[::2]:                                      # each source is shared by the two jobs of its shape
        w.mul_(-1.5).add_(0.25)
    plan.begin()
    torch.cuda.synchronize()
    changed = 0
    for (name, kind, w, stride, pad, old), (_, buf, dst, _) in zip(jobs, held):
        want = _per_tensor(vh, kind, w, stride, pad, dtype).view(torch.int16).reshape(-1)
        changed += int(not torch.equal(want, old))
        assert torch.equal(dst.view(torch.int16), want), name
        assert bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[-GUARD:] == GUARD_BITS).all()), name
        assert plan.lookup(name, w) is dst
    assert changed == len(jobs)
    name, _, w, *_ = jobs[0]
    w.add_(1.0)
    assert plan.lookup(name, w) is None and plan.stale                 # changed since begin(): not honoured
    plan.begin()                                                       # a stale plan records again
    assert not plan.ready and not plan.jobs and not plan.stale


def test_no_jobs_is_a_no_op_and_bad_arguments_are_refused(vh):
    lib = vh.lib()
    assert lib.vatl_pack_weights_h16_multi(None, 0, 0, 1, None) == 0
    some = torch.zeros(64, dtype=torch.uint8, device=dev())
    assert lib.vatl_pack_weights_h16_multi(None, 1, 1, 1, None) != 0
    assert lib.vatl_pack_weights_h16_multi(some.data_ptr(), 1, 1, 2, None) != 0            # neither float16 nor bfloat16
    assert lib.vatl_pack_weights_h16_multi(some.data_ptr(), 1, 0, 1, None) != 0
    plan = vh.PackPlanH16(torch.bfloat16)
    plan.begin()
    plan.seal()
    assert not plan.ready                                              # an empty record is not a plan
    w = torch.zeros(8, 8, 3, 3, device=dev())
    with pytest.raises(vh.VatlError):
        plan.record("short", w, torch.zeros(8 * 8 * 9 - 1, dtype=torch.bfloat16, device=dev()), vh.PACK_H16_CONV)
    with pytest.raises(vh.VatlError):
        plan.record("dtype", w, torch.zeros(8 * 8 * 9, dtype=torch.float16, device=dev()), vh.PACK_H16_CONV)
    with pytest.raises(vh.VatlError):
        plan.record("stride", w, torch.zeros(8 * 8 * 9, dtype=torch.bfloat16, device=dev()), vh.PACK_H16_DGRAD, 3, 1)
    assert not plan.jobs


# ------------------------------------------------------------------------------------------------------ the plan on the trainer
def _model(seed):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = edict({"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50})
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    torch.manual_seed(seed)
    return builder.build_sppe(cfg, preset_cfg=preset)


def test_plan_life_cycle_on_the_r50_trainer(vh, monkeypatch):
    from alphapose.models import hip_train_h16
    assert hip_train_h16._USE_PACK_PLAN is True
    m = _model(3).to(dev()).train()
    x = to_dev(synth.crops(2, seed=31, hw=(96, 64)))
    labels, masks = (to_dev(t) for t in synth.gaussian_targets(2, seed=32, hw=(24, 16)))
    tr = hip_train_h16.trainer_for_h16(m)
    assert len(tr.packed) == 113
    calls = {"conv": 0, "deconv": 0, "dgrad": 0}
    real = {"conv": vh.pack_conv_weight_h16, "deconv": vh.pack_deconv_weight_h16, "dgrad": vh.pack_conv_weight_dgrad_h16}

    def counted(name):
        def inner(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return inner
    monkeypatch.setattr(vh, "pack_conv_weight_h16", counted("conv"))
    monkeypatch.setattr(vh, "pack_deconv_weight_h16", counted("deconv"))
    monkeypatch.setattr(vh, "pack_conv_weight_dgrad_h16", counted("dgrad"))

    def step(between=None):
        with torch.no_grad():
            out = tr.forward(x)
            _, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
            if between is not None:
                between()
            grads = tr.backward(dout)
            for p in m.parameters():
                p.add_(grads[p].reshape(p.shape), alpha=-1e-3)         # in place: the version counters move
        return out

    def kept_are_current():
        for q in tr.packed:
            assert torch.equal(q.get().view(torch.int16).reshape(-1), q.pack(q.p.detach()).view(torch.int16).reshape(-1))

    with torch.no_grad():
        tr.forward(x)                                                  # the recording pass: per-tensor packs, all 113 of them
    plan = tr.__dict__["_pack_plan"]
    assert plan.ready and len(plan.jobs) == 113 and not plan.stale
    assert calls == {"conv": 57 + 3 - 3, "deconv": 3, "dgrad": 56 - 3}, calls          # the three transposed convs: own forward pack, conv pack as data gradient
    with torch.no_grad():
        _, dout = vh.masked_mse_fwd_bwd(tr.forward(x), labels, masks)  # (a forward pass alone leaves no tape that matters: the next one replaces it)
        grads = tr.backward(dout)
        for p in m.parameters():
            p.add_(grads[p].reshape(p.shape), alpha=-1e-3)
    for k in calls:
        calls[k] = 0

    out2 = step()                                                      # the second step: one launch, no per-tensor pack
    assert calls == {"conv": 0, "deconv": 0, "dgrad": 0}, calls
    assert plan.ready and not plan.stale and torch.isfinite(out2).all()
    with torch.no_grad():
        tr.forward(x)                                                  # refreshes the kept buffers from the weights `step` just changed
    assert calls == {"conv": 0, "deconv": 0, "dgrad": 0}, calls
    kept_are_current()                                                 # (calls the per-tensor packers itself)
    for k in calls:
        calls[k] = 0

    head = m.final_layer.weight
    step(between=lambda: torch.autograd.graph.increment_version(head)) # the head's data-gradient filter is read after the bump, with no begin() in between
    assert calls == {"conv": 0, "deconv": 0, "dgrad": 1}, calls        # packed on the spot ...
    assert plan.stale
    with torch.no_grad():
        tr.forward(x)                                                  # ... and the plan records again
    assert plan.ready and not plan.stale and len(plan.jobs) == 113
    assert calls["conv"] == 57 and calls["deconv"] == 3 and calls["dgrad"] == 1 + 56 - 3, calls
    kept_are_current()
    torch.cuda.synchronize()
