"""Training step of SimplePose-R50 at 256x192: the opt-in bf16 trainer (hip_train_h16) beside the fp32 trainer, same process, same batch.

    python tools/train_h16_bench.py [--batches 24,60,120] [--reps 10] [--optimizer {adamw,adam}] [--no-pack-plan] [--out FILE]

A step is forward + masked-MSE loss + backward into the gradient arena + the optimiser (active_learning.optim): AdamW at lr 2.5e-4 / weight
decay 0.7, what ``retrain_model`` runs per mini-batch, or with ``--optimizer adam`` Adam at lr 1e-3, the step of ``alphapose.pretrain``
(whose shipped yaml trains at B = 180).  The bf16 step includes the re-pack of every bf16 filter (the parameters change every step): one
launch under the trainer's pack plan; ``--no-pack-plan`` adds a third route, the bf16 trainer with ``_USE_PACK_PLAN = False`` (113 per-tensor
pack launches, the step before the plan existed), alternated with the other two.  Per batch size: two
warm-up steps per trainer, then ``--reps`` rounds in which the trainers take turns, every step between its own pair of device events.
Reported: the median ms per step of each trainer with its spread (min / max), the ratio, the peak device memory of a step of each
(allocator high-water mark above what is resident before the step: activations, gradients in flight, workspaces), and — from one more
bf16 step on ONE stream (the weight gradients otherwise run on the trainer's side stream) with every kernel-wrapper call between its
own events, which adds an event pair and host time per call, so it is a SPLIT, not a step time — how the device time divides between conv launches (forward, data gradient, weight gradient + its reduction), glue
(BatchNorm passes, pooling, layout conversions, bias gradient) and filter packs.  One JSON line per batch size is appended to ``--out``
(default profiles/train_h16_bench.jsonl) and printed.  A finding to be written down, not a gate: needs an MI355X, fails without one.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
sys.path.insert(0, ROOT)

PIXEL_MEAN = (0.406, 0.457, 0.480)
CONV = ("conv2d_fwd_h16", "deconv4x4s2_fwd_h16", "conv2d_dgrad_h16", "conv2d_wgrad_h16")
PACK = ("pack_conv_weight_h16", "pack_deconv_weight_h16", "pack_conv_weight_dgrad_h16")
GLUE = ("bn_train_fwd_stats_h16", "bn_apply_h16", "bn_train_bwd_h16", "maxpool3x3s2_fwd_h16", "maxpool3x3s2_bwd_h16", "nchw_to_nhwc_h16", "nchw_to_nhwc", "col_sum")


def _build(seed):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = edict({"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50})
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    torch.manual_seed(seed)
    return builder.build_sppe(cfg, preset_cfg=preset)


class _Route:
    """"fp32", "bf16" (the trainer as shipped: one-launch re-pack) or "bf16_unplanned" (every re-pack its own launch)."""

    def __init__(self, name, dev, optimizer="adamw"):
        import vatl_hip as vh
        from active_learning import optim
        from alphapose.models import hip_train, hip_train_h16
        self.vh, self.h16 = vh, hip_train_h16
        self.planned = name != "bf16_unplanned"
        self.m = _build(3).to(dev).train()
        self.tr = hip_train.trainer_for(self.m) if name == "fp32" else hip_train_h16.trainer_for_h16(self.m)
        self.arena = hip_train.arena_for(self.m)
        self.opt = optim.Adam(self.m.parameters(), lr=1e-3) if optimizer == "adam" else optim.AdamW(self.m.parameters(), lr=2.5e-4, weight_decay=0.7)

    def step(self, x, labels, masks):
        keep, self.h16._USE_PACK_PLAN = self.h16._USE_PACK_PLAN, self.planned
        try:
            with torch.no_grad():
                out = self.tr.forward(x)
                loss, dout = self.vh.masked_mse_fwd_bwd(out, labels, masks)
                self.arena.begin()
                self.tr.backward(dout, arena=self.arena)
                self.arena.finish()
                self.arena.attach()
        finally:
            self.h16._USE_PACK_PLAN = keep
        self.opt.step()
        return loss


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def _split(route, x, labels, masks):
    """One bf16 step with every wrapper call of the three classes between its own events -> ms per class and the call counts; the pack
    plan's one refresh launch counts as one pack call."""
    vh = route.vh
    acc = {"conv": [0.0, 0], "glue": [0.0, 0], "pack": [0.0, 0]}
    saved = {}

    def wrap(name, kind):
        fn = saved[name] = getattr(vh, name)

        def timed(*a, **k):
            r, ms = _event_ms(lambda: fn(*a, **k))
            acc[kind][0] += ms
            acc[kind][1] += 1
            return r
        setattr(vh, name, timed)
    from alphapose.models import hip_train
    for kind, names in (("conv", CONV), ("glue", GLUE), ("pack", PACK)):
        for n in names:
            wrap(n, kind)
    begin = vh.PackPlanH16.begin

    def timed_begin(plan):
        launches = plan.ready and not plan.stale
        _, ms = _event_ms(lambda: begin(plan))
        if launches:
            acc["pack"][0] += ms
            acc["pack"][1] += 1
    vh.PackPlanH16.begin = timed_begin
    side, hip_train._side.enabled = hip_train._side.enabled, False        # one stream: a call's events then bracket its own launches
    try:
        _, total = _event_ms(lambda: route.step(x, labels, masks))
    finally:
        hip_train._side.enabled = side
        vh.PackPlanH16.begin = begin
        for n, fn in saved.items():
            setattr(vh, n, fn)
    return acc, total


def bench(b, reps, dev, optimizer="adamw", unplanned=False):
    gen = torch.Generator().manual_seed(b)
    x = (torch.rand((b, 3, 256, 192), generator=gen) - torch.tensor(PIXEL_MEAN).view(1, 3, 1, 1)).to(dev)
    labels = (torch.rand((b, 17, 64, 48), generator=gen) ** 8).to(dev)
    masks = (torch.rand((b, 17, 1, 1), generator=gen) > 0.2).float().to(dev)
    routes = {n: _Route(n, dev, optimizer) for n in ("fp32", "bf16") + (("bf16_unplanned",) if unplanned else ())}
    ms = {n: [] for n in routes}
    peak = {}
    for n, r in routes.items():                                # warm-up: code objects, pack plans, allocator
        for _ in range(2):
            r.step(x, labels, masks)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r.step(x, labels, masks)
        torch.cuda.synchronize()
        peak[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(reps):
        for n, r in routes.items():                            # the trainers take turns, so a drift of the clock meets both
            ms[n].append(_event_ms(lambda: r.step(x, labels, masks))[1])
    row = {"net": "simplepose_r50", "input": [256, 192], "batch": b, "reps": reps, "optimizer": optimizer, "device": torch.cuda.get_device_name(0)}
    for n in routes:
        row[f"step_ms_{n}"] = statistics.median(ms[n])
        row[f"step_ms_{n}_min_max"] = [min(ms[n]), max(ms[n])]
        row[f"step_peak_mib_{n}"] = peak[n]
    row["ratio_fp32_over_bf16"] = row["step_ms_fp32"] / row["step_ms_bf16"]
    for n in (n for n in routes if n != "fp32"):
        _split(routes[n], x, labels, masks)                    # warm the wrappers' path
        acc, total = _split(routes[n], x, labels, masks)
        for kind, (t, k) in acc.items():
            row[f"{n}_{kind}_ms"] = t
            row[f"{n}_{kind}_calls"] = k
        row[f"{n}_split_step_ms"] = total
    if unplanned:
        row["ratio_unplanned_over_planned"] = row["step_ms_bf16_unplanned"] / row["step_ms_bf16"]
    return row


def _sig4(v):
    if isinstance(v, float):
        return float(f"{v:.4g}")
    if isinstance(v, list):
        return [_sig4(x) for x in v]
    return {k: _sig4(x) for k, x in v.items()} if isinstance(v, dict) else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="24,60,120")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--optimizer", choices=("adamw", "adam"), default="adamw", help="adamw: the fine-tune step; adam: the pre-training step (lr 1e-3)")
    ap.add_argument("--no-pack-plan", action="store_true", help="also run the bf16 trainer with every filter re-pack its own launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_h16_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_h16_bench.py measures on an MI355X: no device found (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    for b in (int(t) for t in args.batches.split(",")):
        row = _sig4(bench(b, args.reps, dev, args.optimizer, args.no_pack_plan))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
