#!/usr/bin/env python3
"""Timings behind profiles/dcn_notes.md: the deformable conv2 of a FastPose-50-DCN bottleneck, per layer shape of stages 2 - 4.

    python tools/dcn_bench.py [--batches 256,1024] [--iters 10] [--rounds 3] [--net]
    python tools/dcn_bench.py --backward [--batches 32,120] [--iters 10] [--rounds 3] [--step]

Per shape and batch: the fused deformable launch, conv2_offset, the column route (deform_columns + 1x1 GEMM) and the yardstick — the
plain 3x3 on the implicit GEMM (`vh.conv2d_fwd`, same C, Co, grid and stride: the same MFMA work without the gathers).  Each variant is
`iters` launches between two HIP events; the variants alternate inside a round, `rounds` rounds; median and spread (max - min) over
the rounds.  `--net`: whole FastPose-50-DCN (MODULATED, one deformable group, stages 2 - 4) against plain FastPose-50 through
hip_engine.forward_into.  Prints one JSON line per measurement.

`--backward`: the backward of the column matrix (`vh.deform_columns_bwd`) per shape, at the fine-tune batch sizes: the atomic entry
(the default) against the ordered, bit-reproducible entry, same protocol.  The ordered entry is one call of seven launches, so its split
comes from a kernel trace taken afterwards (torch.profiler, a pass of its own, `iters` calls): the index build (count, scan, fill,
sort and the memset of the counts), the sum pass, and the d_offset / d_mask kernel.  `--step`: one FastPose-50-DCN fine-tune step
(forward, loss, backward into the arena, AdamW) with the switch off and on.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import vatl_hip as vh  # noqa: E402

# name: (H, W, C, stride) of conv2's input at 256x192 crops; Co = C
SHAPES = {"l2.0": (64, 48, 128, 2), "l2.n": (32, 24, 128, 1), "l3.0": (32, 24, 256, 2), "l3.n": (16, 12, 256, 1),
          "l4.0": (16, 12, 512, 2), "l4.n": (8, 6, 512, 1)}


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / iters


def alternate(variants, iters, rounds):
    for fn in variants.values():                       # warm-up: code objects, allocator
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    return {k: {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "runs_ms": [round(t, 4) for t in v]} for k, v in times.items()}


def layer(name, batch, iters, rounds, dev):
    h, w, c, s = SHAPES[name]
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn((batch, h, w, c), generator=g).to(dev)
    wt = (torch.randn((c, c, 3, 3), generator=g) / (9 * c) ** 0.5).to(dev)
    woff = (0.05 * torch.randn((27, c, 3, 3), generator=g) / (9 * c) ** 0.5 * 9).to(dev)      # offsets of about half a pixel
    boff = torch.zeros(27, device=dev)
    scale, bias = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    wp, wo_p, wd, wg = vh.pack_conv_weight(wt), vh.pack_conv_weight(woff), vh.pack_deform_weight(wt), vh.pack_conv_weight(vh.deform_gemm_weight(wt))
    _, ob = vh.bn_fold(None, None, None, None, 0.0, boff, channels=27)
    om = vh.conv2d_fwd(x, wo_p, None, ob, 27, 3, 3, s, 1, False)
    ho, wo = om.shape[1], om.shape[2]
    y = torch.empty((batch, ho, wo, c), device=dev)

    def columns():
        col = vh.deform_columns(x, om, True, s, 1)
        vh.conv2d_fwd(col, wg, scale, bias, c, 1, 1, 1, 0, True, out=y)
    variants = {
        "fused": lambda: vh.deform_conv2d_fwd(x, wd, om, True, scale, bias, s, 1, True, out=y),
        "offset_conv": lambda: vh.conv2d_fwd(x, wo_p, None, ob, 27, 3, 3, s, 1, False, out=om),
        "columns_gemm": columns,
        "yardstick_conv3x3": lambda: vh.conv2d_fwd(x, wp, scale, bias, c, 3, 3, s, 1, True, out=y),
    }
    res = alternate(variants, iters, rounds)
    gflop = 2.0 * batch * ho * wo * 9 * c * c / 1e9
    print(json.dumps({"layer": name, "batch": batch, "in": [h, w, c], "stride": s, "gflop": round(gflop, 2), **res}), flush=True)


def net(batch, rounds, dev):
    from alphapose.models import builder, hip_engine
    from alphapose.utils.config import edict
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    base = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
    torch.manual_seed(0)
    plain = builder.build_sppe(edict(base), preset_cfg=preset).to(dev).eval()
    dcn = builder.build_sppe(edict({**base, "DCN": {"MODULATED": True, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False},
                                    "STAGE_WITH_DCN": [False, True, True, True]}), preset_cfg=preset).to(dev).eval()
    with torch.no_grad():
        for m in dcn.modules():
            if hasattr(m, "conv2_offset"):
                m.conv2_offset.weight.mul_(0.05)
    x = torch.randn((batch, 3, 256, 192), device=dev)
    hm = torch.empty((batch, 17, 64, 48), device=dev)
    with torch.no_grad():
        res = alternate({"fastpose50": lambda: hip_engine.forward_into(plain, x, hm), "fastpose50_dcn": lambda: hip_engine.forward_into(dcn, x, hm)}, 3, rounds)
    print(json.dumps({"net": "FastPose-50 forward", "batch": batch, **res}), flush=True)


def backward(name, batch, iters, rounds, dev):
    h, w, c, s = SHAPES[name]
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn((batch, h, w, c), generator=g).to(dev)
    woff = (0.05 * torch.randn((27, c, 3, 3), generator=g) / (9 * c) ** 0.5 * 9).to(dev)      # offsets of about half a pixel, as layer()
    _, ob = vh.bn_fold(None, None, None, None, 0.0, torch.zeros(27, device=dev), channels=27)
    om = vh.conv2d_fwd(x, vh.pack_conv_weight(woff), None, ob, 27, 3, 3, s, 1, False)
    ho, wo = om.shape[1], om.shape[2]
    dcol = torch.zeros((batch, ho, wo, vh.deform_col_stride(c)), device=dev)
    dcol[..., :9 * c] = torch.randn((batch, ho, wo, 9 * c), generator=g).to(dev)
    variants = {"atomic": lambda: vh.deform_columns_bwd(dcol, x, om, True, s, 1, grad_channels=32, deterministic=False),
                "ordered": lambda: vh.deform_columns_bwd(dcol, x, om, True, s, 1, grad_channels=32, deterministic=True)}
    res = alternate(variants, iters, rounds)
    res["ordered_over_atomic"] = round(res["ordered"]["median_ms"] / res["atomic"]["median_ms"], 3)
    # the split of the ordered entry: device time per kernel over `iters` calls, in a pass of its own
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            variants["ordered"]()
        torch.cuda.synchronize()
    split = {"index_build": 0.0, "sum_pass": 0.0, "d_offset_d_mask": 0.0, "other": 0.0}
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None)
        if us is None:
            us = ev.cuda_time_total
        if not us:
            continue
        if "deform_dx_sum" in ev.key:
            split["sum_pass"] += us
        elif "deform_columns_bwd" in ev.key:
            split["d_offset_d_mask"] += us
        elif "deform_index" in ev.key or "memset" in ev.key.lower() or "fillbuffer" in ev.key.lower():
            split["index_build"] += us
        else:
            split["other"] += us                       # torch's zero fill of d_offset
    if not (split["sum_pass"] and split["index_build"]):
        raise RuntimeError("the kernel trace holds no deformable kernels: " + ", ".join(ev.key for ev in prof.key_averages()))
    res["ordered_split_ms"] = {k: round(v / iters / 1e3, 4) for k, v in split.items()}
    print(json.dumps({"backward": name, "batch": batch, "in": [h, w, c], "stride": s, **res}), flush=True)


def step(batch, rounds, dev):
    from active_learning.optim import AdamW
    from alphapose.models import builder, hip_train
    from alphapose.models.layers import dcn
    from alphapose.utils.config import edict
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    torch.manual_seed(0)
    m = builder.build_sppe(edict({"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50,
                                  "DCN": {"MODULATED": True, "DEFORM_GROUP": 1, "FALLBACK_ON_STRIDE": False},
                                  "STAGE_WITH_DCN": [False, True, True, True]}), preset_cfg=preset).to(dev).train()
    with torch.no_grad():
        for mod in m.modules():
            if hasattr(mod, "conv2_offset"):
                mod.conv2_offset.weight.mul_(0.05)
    opt = AdamW(params=[{"params": m.parameters(), "lr": 1e-5}], weight_decay=0.7)
    x = torch.rand((batch, 3, 256, 192), device=dev) - 0.45
    labels = torch.rand((batch, 17, 64, 48), device=dev) * 0.1
    masks = (torch.rand((batch, 17, 1, 1), device=dev) > 0.2).float()
    tr, arena = hip_train.trainer_for(m), hip_train.arena_for(m)

    def one(mode):
        with dcn.deterministic(mode), torch.no_grad():
            out = tr.forward(x)
            _, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
            arena.begin()
            tr.backward(dout, arena=arena, overlap=True)
            arena.finish()
            arena.attach()
        opt.step()
    res = alternate({"atomic": lambda: one(False), "ordered": lambda: one(True)}, 3, rounds)
    res["ordered_over_atomic"] = round(res["ordered"]["median_ms"] / res["atomic"]["median_ms"], 3)
    print(json.dumps({"net": "FastPose-50-DCN fine-tune step", "batch": batch, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", default=",".join(SHAPES))
    ap.add_argument("--net", action="store_true")
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if a.batches is None:
        a.batches = "32,120" if a.backward else "256,1024"
    dev = torch.device("cuda:0")
    warm = torch.randn((4096, 4096), device=dev)       # clock warm-up: the first configuration of a fresh process otherwise reads slow
    for _ in range(20):
        warm = torch.tanh(warm @ warm * 1e-4)
    torch.cuda.synchronize()
    for b in [int(v) for v in a.batches.split(",")]:
        for name in [n for n in a.layers.split(",") if n]:
            (backward if a.backward else layer)(name, b, a.iters, a.rounds, dev)
        if a.net:
            net(b, a.rounds, dev)
        if a.step:
            step(b, a.rounds, dev)


if __name__ == "__main__":
    main()
