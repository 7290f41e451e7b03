"""Arg-max flip rate of the timed fp32 stream route against the float64 reference ON THE DEVICE, on thousands of fresh crops.

    python tools/flip_rate.py --net simplepose_r50|fastpose_r50|hrnet_w32|fastpose_r152_384 [--crops N] [--seed S] [--out FILE]
                              [--route stream|fp16|bf16]

``--route fp16`` / ``bf16`` judges the opt-in 16-bit route (``hip_engine_h16.forward_h16``) instead of the stream route, against the same
float64 reference on the same crops: the same fields (``crops_per_s_route`` and ``idx_route`` in place of the ``fp32`` names), plus
``route`` and ``nonfinite_planes`` (planes of the route that hold an inf or a NaN), appended to profiles/h16_flips.jsonl by default; its flipped
planes are counted, not listed one by one.

The model gets torch's default initialisation under ``--seed``, BatchNorm running statistics are randomised (mean 0.1 * N(0,1), variance
U(0.5, 1.5)), crops are ``rand - pixel mean``.  Both routes run on the same crops, block by block: ``hip_engine.forward_into`` (the route
bench.py times) and ``hip_engine_f64.forward_f64``.  One JSON line is appended to ``--out`` (default profiles/f64_reference_flips.jsonl):

  planes, flipped          joint planes seen / planes whose arg-max index differs between the two routes
  flips                    per flipped plane: crop, joint, both indices and the float64 top-2 gap relative to the plane's range (max - min)
  min_gap_rel              the smallest such relative gap met over ALL planes
  route_rel_err            max |fp32 - float64| / max |float64| over everything (tests.gpu_util.rel_err's definition)
  crops_per_s_fp32, crops_per_s_f64   device time between synchronisations; the float64 figure includes packing the filters once per block
  host_*                   the same network in float64 with torch on the host, 16 crops, once, at most 16 threads: its crops/s, and how far
                           the device reference is from it (normwise distance, planes whose arg-max differs)

A finding to be written down, not a gate: nothing here changes a route.  Defaults: 4096 crops (512 for the 384x288 network).
"""
import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
sys.path.insert(0, ROOT)

PIXEL_MEAN = (0.406, 0.457, 0.480)
_HR = lambda mods, ch: {"NUM_MODULES": mods, "NUM_BRANCHES": len(ch), "NUM_BLOCKS": [4] * len(ch), "NUM_CHANNELS": ch, "BLOCK": "BASIC", "FUSE_METHOD": "SUM"}
NETS = {   # name: (MODEL cfg, input size, default crops)
    "simplepose_r50": ({"TYPE": "SimplePose", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}, (256, 192), 4096),
    "fastpose_r50": ({"TYPE": "FastPose", "NUM_LAYERS": 50}, (256, 192), 4096),
    "hrnet_w32": ({"TYPE": "PoseHighResolutionNet", "NUM_LAYERS": 50, "FINAL_CONV_KERNEL": 1, "PRETRAINED_LAYERS": ["*"],
                   "STAGE2": _HR(1, [32, 64]), "STAGE3": _HR(4, [32, 64, 128]), "STAGE4": _HR(3, [32, 64, 128, 256])}, (256, 192), 4096),
    "fastpose_r152_384": ({"TYPE": "FastPose", "NUM_LAYERS": 152}, (384, 288), 512),
}
BLOCK = 512          # crops generated, uploaded and run at a time
MAX_LISTED = 512     # flipped planes listed one by one (the count is always complete)
MAX_LISTED_H16 = 0    # ... of a 16-bit route, which flips thousands of near-ties: counted, not listed


def build(name, seed):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg, hw, _ = NETS[name]
    torch.manual_seed(seed)
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": list(hw), "HEATMAP_SIZE": [hw[0] // 4, hw[1] // 4]})
    m = builder.build_sppe(edict(dict({"PRETRAINED": "", "TRY_LOAD": ""}, **cfg)), preset_cfg=preset)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features))
    return m.eval()


# ------------------------------------------------------------------------------------------- the host float64 path (torch, CPU)
def _cbr(x, conv, bn, relu):
    x = bn(conv(x))
    return F.relu(x) if relu else x


def _host_block(b, x):
    last = 3 if hasattr(b, "conv3") else 2
    y = x
    for k in range(1, last + 1):
        y = _cbr(y, getattr(b, f"conv{k}"), getattr(b, f"bn{k}"), k < last)
    if getattr(b, "reduc", False):
        y = y * b.se.fc(y.mean(dim=(2, 3)))[:, :, None, None]
    return F.relu(y + (x if b.downsample is None else b.downsample(x)))


def _host_trunk(net, x):
    x = net.maxpool(_cbr(x, net.conv1, net.bn1, True))
    for stage in net.stages():
        for b in stage:
            x = _host_block(b, x)
    return x


def _host_hr_module(mod, xs):
    xs = list(xs)
    for i, br in enumerate(mod.branches):
        for b in br:
            xs[i] = _host_block(b, xs[i])
    if mod.fuse_layers is None:
        return xs
    out = []
    for i, row in enumerate(mod.fuse_layers):
        y = xs[0] if i == 0 else row[0](xs[0])
        for j in range(1, len(xs)):
            y = y + (xs[j] if i == j else row[j](xs[j]))
        out.append(F.relu(y))
    return out


def host_forward(m, x):
    """``m``: a float64 copy of the model on the host.  Its containers hold standard torch layers: they are called one by one."""
    kind = type(m).__name__
    if kind == "SimplePose":
        return m.final_layer(m.deconv_layers(_host_trunk(m.preact, x)))
    if kind == "FastPose":
        x = m.suffle1(_host_trunk(m.preact, x))
        for duc in (m.duc1, m.duc2):
            x = duc.pixel_shuffle(_cbr(x, duc.conv, duc.bn, True))
        return m.conv_out(x)
    x = _cbr(_cbr(x, m.conv1, m.bn1, True), m.conv2, m.bn2, True)
    for b in m.layer1:
        x = _host_block(b, x)
    ys = [x]
    for s in (2, 3, 4):
        xs = [ys[i] if t is None else t(ys[-1]) for i, t in enumerate(getattr(m, f"transition{s - 1}"))]
        for mod in getattr(m, f"stage{s}"):
            xs = _host_hr_module(mod, xs)
        ys = xs
    return m.final_layer(ys[0])


def _timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", required=True, choices=list(NETS))
    ap.add_argument("--crops", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--route", default="stream", choices=["stream", "fp16", "bf16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    h16 = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(args.route)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "f64_reference_flips.jsonl" if h16 is None else "h16_flips.jsonl")
    from alphapose.models import hip_engine, hip_engine_f64, hip_engine_h16
    route = hip_engine.forward_into if h16 is None else (lambda mod, t, out: hip_engine_h16.forward_h16(mod, t, out, dtype=h16))
    tag = "fp32" if h16 is None else "route"
    cfg, hw, default_crops = NETS[args.net]
    n = args.crops or default_crops
    dev = torch.device("cuda:0")
    m = build(args.net, args.seed)
    host = copy.deepcopy(m).double()
    m = m.to(dev)
    gen = torch.Generator().manual_seed(args.seed + 1)
    mean = torch.tensor(PIXEL_MEAN).view(1, 3, 1, 1)
    hm_hw = (hw[0] // 4, hw[1] // 4)

    t32 = t64 = 0.0
    planes = flipped = nonfinite = 0
    flips = []
    min_gap_rel, max_diff, max_ref = float("inf"), 0.0, 0.0
    first = None
    with torch.no_grad():
        for a in range(0, n, BLOCK):
            b = min(a + BLOCK, n)
            x_host = torch.rand((b - a, 3) + hw, generator=gen) - mean
            x = x_host.to(dev)
            out32 = torch.empty((b - a, 17) + hm_hw, device=dev)
            if a == 0:                                              # plan build, lazy filter packs, library load: not timed
                route(m, x[:8], out32[:8])
                hip_engine_f64.forward_f64(m, x[:2])
            _, dt = _timed(lambda: route(m, x, out32))
            t32 += dt
            h64, dt = _timed(lambda: hip_engine_f64.forward_f64(m, x))
            t64 += dt
            if a == 0:
                first = (x_host[:16].clone(), h64[:16].cpu())
            f64 = h64.flatten(2)
            i32, i64 = out32.flatten(2).argmax(2), f64.argmax(2)
            top = f64.topk(2, dim=2).values
            gap_rel = (top[..., 0] - top[..., 1]) / (f64.amax(2) - f64.amin(2)).clamp_min(1e-300)
            planes += i64.numel()
            nonfinite += int((~torch.isfinite(out32).flatten(2).all(2)).sum())
            min_gap_rel = min(min_gap_rel, float(gap_rel.min()))
            max_diff = max(max_diff, float((out32.double() - h64).abs().max()))
            max_ref = max(max_ref, float(h64.abs().max()))
            for c, j in torch.nonzero(i32 != i64).tolist():
                flipped += 1
                if len(flips) < (MAX_LISTED if h16 is None else MAX_LISTED_H16):
                    flips.append({"crop": a + c, "joint": j, f"idx_{tag}": int(i32[c, j]), "idx_f64": int(i64[c, j]), "gap_rel": float(gap_rel[c, j])})
            del x, out32, h64, f64, top, gap_rel

    # the host float64 path, once, on 16 crops
    threads = min(16, torch.get_num_threads())
    torch.set_num_threads(threads)
    xh, dev16 = first
    t = time.perf_counter()
    with torch.no_grad():
        h_host = host_forward(host, xh.double())
    t_host = time.perf_counter() - t
    k = xh.shape[0]
    host_rel = float((dev16 - h_host).abs().max() / h_host.abs().max())
    host_moved = int((dev16.flatten(2).argmax(2) != h_host.flatten(2).argmax(2)).sum())

    row = {"net": args.net, "input": list(hw), "crops": n, "block": BLOCK, "seed": args.seed, "planes": planes, "flipped": flipped, "flip_rate": flipped / planes,
           "flips": flips, "flips_listed": len(flips), "min_gap_rel": min_gap_rel, "route_rel_err": max_diff / max_ref,
           f"crops_per_s_{tag}": n / t32, "crops_per_s_f64": n / t64, "host_crops": k, "host_threads": threads, "host_crops_per_s": k / t_host,
           "device_f64_over_host_f64": (n / t64) / (k / t_host), "device_f64_vs_host_rel_err": host_rel, "device_f64_vs_host_argmax_moved": host_moved,
           "device": torch.cuda.get_device_name(0)}
    if h16 is not None:
        row = dict(row, route=args.route, nonfinite_planes=nonfinite)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps({k2: v for k2, v in row.items() if k2 != "flips"}))


if __name__ == "__main__":
    main()
