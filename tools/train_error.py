"""How far the two trainers' gradients are from float64, per tensor, at the sizes the product runs: SimplePose-R50 at 256x192.

    python tools/train_error.py [--batches 24,60,120] [--limit 600] [--out FILE]

Per batch size, from ONE seeded default initialisation and one seeded batch (crops, Gaussian targets, joint masks), three steps run
from the same state: the fp32 trainer (``hip_train``), the bf16 trainer (``hip_train_h16``) and the float64 reference on the device
(``hip_train_f64``).  Each takes the cotangent of the masked 0.5 * MSE the fine-tune step uses from its OWN heat-maps, as a real step
does.  Written per batch size, one JSON line appended to ``--out`` (default profiles/train_f64_error.jsonl) and printed:
  * per parameter tensor the normwise distance |g - g64| / |g64| of each trainer's gradient from the float64 one;
  * the same for the heat-maps and, per BatchNorm layer, for the running mean / variance the step writes (float64: would write);
  * the float64 step's device time (forward + backward, warm, device events) and the peak device memory of that step.
Each batch size runs in a child process of its own under ``timeout``; the script stops at the first one that fails.  A finding to be
written down, not a gate: needs an MI355X, fails without one.
"""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
sys.path.insert(0, ROOT)

PIXEL_MEAN = (0.406, 0.457, 0.480)
HW, HM, JOINTS = (256, 192), (64, 48), 17


def _build(seed):
    import torch
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = edict({"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50})
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": JOINTS, "IMAGE_SIZE": list(HW), "HEATMAP_SIZE": list(HM)})
    torch.manual_seed(seed)
    return builder.build_sppe(cfg, preset_cfg=preset)


def _batch(b, seed):
    """Seeded crops (mean-subtracted uniform pixels), Gaussian targets (sigma 2) at seeded joint positions, seeded 0 / 1 joint masks."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((b, 3, *HW), generator=g) - torch.tensor(PIXEL_MEAN).reshape(1, 3, 1, 1)
    cy = torch.rand((b, JOINTS, 1, 1), generator=g) * HM[0]
    cx = torch.rand((b, JOINTS, 1, 1), generator=g) * HM[1]
    ys, xs = torch.arange(HM[0]).reshape(1, 1, -1, 1), torch.arange(HM[1]).reshape(1, 1, 1, -1)
    labels = torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * 2.0 ** 2))
    masks = (torch.rand((b, JOINTS), generator=g) > 0.2).float()
    return x, labels.contiguous(), masks


def _dist(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _summary(v):
    import statistics
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def worker(b):
    import torch
    import vatl_hip as vh
    from alphapose.models import hip_train, hip_train_f64, hip_train_h16
    dev = torch.device("cuda:0")
    base = _build(3).to(dev).train()
    x, labels, masks = (t.to(dev) for t in _batch(b, 7))
    names = [k for k, _ in base.named_parameters()]
    bns = [k for k, mod in base.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]

    # the float64 reference: one warm-up pass, then the timed one (two passes from one state are bit-equal)
    tr64 = hip_train_f64.trainer_for_f64(base)
    m4 = masks.double().reshape(b, JOINTS, 1, 1)

    def step64():
        out = tr64.forward(x)
        dout = ((out - labels.double()) * m4 * m4 / out.numel()).contiguous()          # d/d out of 0.5 * mean((out*m - target*m)^2)
        return out, tr64.backward(dout)

    step64()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    resident = torch.cuda.memory_allocated()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out64, g64 = step64()
    t1.record()
    torch.cuda.synchronize()
    rec = {"batch": b, "net": "simplepose_r50", "hw": list(HW), "f64_step_ms": t0.elapsed_time(t1),
           "f64_step_peak_gib": (torch.cuda.max_memory_allocated() - resident) / 2 ** 30}
    named64 = dict(base.named_parameters())
    g64 = {k: g64[named64[k]] for k in names}
    mods64 = dict(base.named_modules())
    stats64 = tr64.batch_statistics()
    st64 = {k: stats64[mods64[k]] for k in bns}

    tensors = {k: {} for k in names}
    for route, get in (("fp32", hip_train.trainer_for), ("bf16", hip_train_h16.trainer_for_h16)):
        m = copy.deepcopy(base).train()                                               # the same state; this trainer updates its running statistics
        tr = get(m)
        with torch.no_grad():
            out = tr.forward(x)
            _, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
            grads = tr.backward(dout)
        torch.cuda.synchronize()
        named, mods = dict(m.named_parameters()), dict(m.named_modules())
        for k in names:
            tensors[k][route] = _dist(grads[named[k]].reshape(g64[k].shape), g64[k])
        rec[f"heatmaps_{route}"] = _dist(out, out64)
        rec[f"gradients_{route}"] = _summary([tensors[k][route] for k in names])
        rec[f"running_mean_{route}"] = _summary([_dist(mods[k].running_mean, st64[k]["running_mean"]) for k in bns])
        rec[f"running_var_{route}"] = _summary([_dist(mods[k].running_var, st64[k]["running_var"]) for k in bns])
        del tr, grads, m
        torch.cuda.empty_cache()
    rec["tensors"] = tensors
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="24,60,120")
    ap.add_argument("--limit", type=int, default=600, help="seconds per batch size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_f64_error.jsonl"))
    ap.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    for b in (int(s) for s in a.batches.split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", str(b)], capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"batch {b}: the step exited with {r.returncode}; stopping")
        rec = json.loads(lines[-1][7:])
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps({k: v for k, v in rec.items() if k != "tensors"}), flush=True)


if __name__ == "__main__":
    main()
