"""Throughput of the opt-in 16-bit inference route (hip_engine_h16) beside the fp32 stream route, in the same run on the same crops.

    python tools/h16_bench.py [--nets simplepose_r50,fastpose_r50,hrnet_w32,fastpose_r152_384] [--crops 512] [--reps 5] [--out FILE]

Per network (those of profiles/f64_reference_notes.md §4; the model and crops are tools/flip_rate.py's): 512 crops per call, one warm-up
call per route, then ``--reps`` rounds in which the three routes take turns (stream fp32, fp16, bf16), each call timed with device events.
Reported: the median crops/s per route and its spread (min / max over the rounds), the ratio to the stream route, the 16-bit filter pack
alone (plan construction: every conv's filter converted and laid out, BatchNorm folded) as milliseconds and as a share of a call — the
route packs on every call, so the call times INCLUDE it.

For SimplePose-R50 additionally the ten layer shapes with the most FLOPs of one 512-crop fp16 and bf16 call, every launch timed with its own
pair of events and summed per shape (a call runs in chunks and a shape recurs in a stage; the phases of a transposed conv are one launch
here): time, direct-sum TFLOP/s (2 * M * Cout * K over the time), and the bytes the launches must move (input, filter and output once each)
over the time; ``conv_ms_*`` is the sum over ALL conv launches of the call, so the rest of the call is glue, packing and launch gaps.  One JSON line per network is appended to ``--out`` (default
profiles/h16_bench.jsonl) and printed.  A finding to be written down, not a gate: needs an MI355X, fails without one.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flip_rate as FR  # noqa: E402  (tools/flip_rate.py: NETS, build, PIXEL_MEAN)

ROUTES = ("fp32", "fp16", "bf16")
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def _layers(m, x, dt):
    """One call with every conv / deconv launch between its own events: [(label, ms, flops, bytes)] in launch order."""
    import vatl_hip as vh
    from alphapose.models import hip_engine_h16
    rows, conv, deconv = [], vh.conv2d_fwd_h16, vh.deconv4x4s2_fwd_h16

    def timed_conv(xx, w, scale, bias, stride, pad, relu, residual=None, out_f32_nchw=False, out=None):
        y, ms = _event_ms(lambda: conv(xx, w, scale, bias, stride, pad, relu, residual=residual, out_f32_nchw=out_f32_nchw, out=out))
        n, h, ww, cin = xx.shape
        cout, r, s, _ = w.shape
        pix = y.numel() // cout
        nbytes = xx.numel() * 2 + w.numel() * 2 + y.numel() * y.element_size() + (0 if residual is None else residual.numel() * 2)
        rows.append((f"conv {r}x{s}/{stride} {cin}->{cout} on {h}x{ww}", ms, 2.0 * pix * cout * r * s * cin, nbytes))
        return y

    def timed_deconv(xx, w, scale, bias, relu):
        y, ms = _event_ms(lambda: deconv(xx, w, scale, bias, relu))
        n, h, ww, cin = xx.shape
        cout = w.shape[1]
        rows.append((f"deconv 4x4/2 {cin}->{cout} on {h}x{ww}", ms, 2.0 * y.numel() * 4 * cin, xx.numel() * 2 + w.numel() * 2 + y.numel() * 2))
        return y

    vh.conv2d_fwd_h16, vh.deconv4x4s2_fwd_h16 = timed_conv, timed_deconv
    try:
        hip_engine_h16.forward_h16(m, x, dtype=dt)
        torch.cuda.synchronize()
    finally:
        vh.conv2d_fwd_h16, vh.deconv4x4s2_fwd_h16 = conv, deconv
    return rows


def bench(name, crops, reps):
    from alphapose.models import hip_engine, hip_engine_h16
    cfg, hw, _ = FR.NETS[name]
    dev = torch.device("cuda:0")
    m = FR.build(name, 0).to(dev)
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand((crops, 3) + hw, generator=gen) - torch.tensor(FR.PIXEL_MEAN).view(1, 3, 1, 1)).to(dev)
    out = torch.empty((crops, 17, hw[0] // 4, hw[1] // 4), device=dev)
    calls = {"fp32": lambda: hip_engine.forward_into(m, x, out),
             "fp16": lambda: hip_engine_h16.forward_h16(m, x, out, dtype=torch.float16),
             "bf16": lambda: hip_engine_h16.forward_h16(m, x, out, dtype=torch.bfloat16)}
    ms = {r: [] for r in ROUTES}
    pack = {r: [] for r in DT}
    with torch.no_grad():
        for r in ROUTES:                                   # warm-up: code objects, plans of the fp32 route, allocator
            calls[r]()
        torch.cuda.synchronize()
        for _ in range(reps):
            for r in ROUTES:                               # the routes take turns, so a drift of the clock meets all of them
                ms[r].append(_event_ms(calls[r])[1])
            for r, dt in DT.items():
                pack[r].append(_event_ms(lambda: hip_engine_h16._net_plan(m, dt))[1])
        row = {"net": name, "input": list(hw), "crops": crops, "reps": reps, "device": torch.cuda.get_device_name(0)}
        base = statistics.median(ms["fp32"])
        for r in ROUTES:
            med = statistics.median(ms[r])
            row[f"crops_per_s_{r}"] = crops / med * 1e3
            row[f"crops_per_s_{r}_min_max"] = [crops / max(ms[r]) * 1e3, crops / min(ms[r]) * 1e3]
            row[f"call_ms_{r}"] = med
            if r != "fp32":
                row[f"ratio_{r}_over_fp32"] = base / med
                row[f"pack_ms_{r}"] = statistics.median(pack[r])
                row[f"pack_share_of_call_{r}"] = statistics.median(pack[r]) / med
        if name == "simplepose_r50":
            for r, dt in DT.items():
                _layers(m, x, dt)                          # warm
                agg = {}                                   # a call runs in chunks, and a layer shape recurs: one entry per shape, its launches summed
                for lab, t, fl, nb in _layers(m, x, dt):
                    a = agg.setdefault(lab, [0, 0.0, 0.0, 0.0])
                    a[0] += 1; a[1] += t; a[2] += fl; a[3] += nb
                rows = sorted(agg.items(), key=lambda kv: -kv[1][2])[:10]
                row[f"layers_{r}"] = [{"layer": lab, "launches": k, "ms": t, "tflops": fl / t / 1e9, "gbytes_per_s": nb / t / 1e6} for lab, (k, t, fl, nb) in rows]
                row[f"conv_ms_{r}"] = sum(a[1] for a in agg.values())
    return row


def _sig4(v):
    """Four significant digits: what these measurements carry."""
    if isinstance(v, float):
        return float(f"{v:.4g}")
    if isinstance(v, list):
        return [_sig4(x) for x in v]
    return {k: _sig4(x) for k, x in v.items()} if isinstance(v, dict) else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default=",".join(FR.NETS))
    ap.add_argument("--crops", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h16_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("h16_bench.py measures on an MI355X: no device found (there is no CPU fallback)")
    for name in args.nets.split(","):
        row = _sig4(bench(name, args.crops, args.reps))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
