#!/usr/bin/env python3
"""The fine-tune step at the batch sizes active learning runs it, eager against the opt-in graphed step (alphapose/models/hip_train_graph.py),
and HRNet's SGD step per tensor against one launch per group.

    python tools/train_graph_bench.py [--configs simple_fp32,simple_bf16,fast_fp32,hrnet_fp32] [--batches 8,24,60,120]
                                      [--repeats 5] [--steps 20] [--linear] [--eager-only] [--root DIR]
    python tools/train_graph_bench.py --sgd [--repeats 5] [--steps 20]

Per (configuration, B) two models are built from one seed with an optimiser each (SimplePose / FastPose: AdamW, three / one groups as
the active-learning loop builds them; HRNet-W32: SGD with momentum).  One takes the eager sequence of ``retrain_model``, the other
``graphed_step_for``; both see the same seeded ``torch.rand`` batches (a pool of four, cycled, so a replay gets other inputs every step).
The two legs alternate in one process, ``--repeats`` times ``--steps`` steps each, a host clock around work that ends in a synchronise.
One line per repeat: ms/step of both legs, vatl_hip wrapper calls per step of both (counted in one extra, untimed step: the counting of
tools/step_calls.py without its synchronises), and whether parameters, buffers and losses of the two models are equal.  A summary line
per (configuration, B) follows: minimum and median of each leg.

``--eager-only`` runs the eager leg alone and imports nothing a tree without the graphed step lacks; with ``--root DIR`` the package and
its library come from another checkout (built there) — how the parent commit's step is measured by the same tool in the same GPU
visit.  ``--linear`` captures single-stream graphs (hip_train_graph.SIDE_STREAM_IN_GRAPH = False).
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="simple_fp32,simple_bf16,fast_fp32,hrnet_fp32")
ap.add_argument("--batches", default="8,24,60,120")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--linear", action="store_true")
ap.add_argument("--eager-only", action="store_true")
ap.add_argument("--sgd", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
for p in (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bench  # noqa: E402
import vatl_hip as vh  # noqa: E402
from active_learning import optim as O  # noqa: E402
from alphapose.models import hip_train  # noqa: E402

HW = (256, 192)
FAST_R50 = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50}
CONFIGS = {                                         # name -> (network config, precision, optimiser)
    "simple_fp32": (bench.SIMPLE_R50, "fp32", "adamw3"),
    "simple_bf16": (bench.SIMPLE_R50, "bf16", "adamw3"),
    "fast_fp32": (FAST_R50, "fp32", "adamw"),
    "hrnet_fp32": (bench.HRNET_W32, "fp32", "sgd"),
}
dev = torch.device("cuda:0")
tag = os.path.basename(ROOT) if args.root != ap.get_default("root") else "this"


def optimiser(m, which):
    if which == "adamw3":
        groups = [{"params": getattr(m, a).parameters(), "lr": 2.5e-4 * f} for a, f in (("final_layer", 10), ("preact", 1), ("deconv_layers", 5))]
        return O.AdamW(params=groups, weight_decay=0.7)
    if which == "adamw":
        return O.AdamW(m.parameters(), lr=2.5e-4, weight_decay=0.7)
    return O.SGD(m.parameters(), lr=2.5e-4, momentum=0.9, weight_decay=5e-4)


def batches(b, n=4):
    g = torch.Generator(device=dev); g.manual_seed(1)
    out = []
    for _ in range(n):
        x = torch.rand((b, 3, HW[0], HW[1]), device=dev, generator=g) - 0.45
        labels = torch.rand((b, 17, HW[0] // 4, HW[1] // 4), device=dev, generator=g) * 0.1
        masks = (torch.rand((b, 17, 1, 1), device=dev, generator=g) > 0.2).float()
        out.append((x, labels, masks))
    return out


def eager_leg(m, precision, opt):
    if precision == "bf16":
        from alphapose.models import hip_train_h16
        tr = hip_train_h16.trainer_for_h16(m)
    else:
        tr = hip_train.trainer_for(m)
    arena = hip_train.arena_for(m)

    def step(x, labels, masks):
        with torch.no_grad():
            out = tr.forward(x)
            loss, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
            arena.begin()
            tr.backward(dout, arena=arena, overlap=True)
            arena.finish()
        arena.attach()
        opt.step()
        return loss.reshape(())
    return step


def graphed_leg(m, precision, opt):
    from alphapose.models import hip_train_graph
    hip_train_graph.SIDE_STREAM_IN_GRAPH = not args.linear
    gs = hip_train_graph.graphed_step_for(m, precision)
    arena = hip_train.arena_for(m)

    def step(x, labels, masks):
        _, loss = gs(x, labels, masks)
        arena.attach()
        opt.step()
        return loss
    step.graphed = gs
    return step


class Leg:
    def __init__(self, fn, pool):
        self.fn, self.pool, self.k, self.loss = fn, pool, 0, None

    def run(self, n):
        for _ in range(n):
            self.loss = self.fn(*self.pool[self.k % len(self.pool)])
            self.k += 1

    def timed(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3


SKIP = {"lib", "upload", "tune_set", "set_pack_plan", "latency_mode", "conv_cout_pad", "enable_splitk"}


def wrapper_calls(leg):
    """vatl_hip wrapper calls of one (untimed) step of ``leg``."""
    count, kept = [0], {}
    for name in dir(vh):
        f = getattr(vh, name)
        if name.startswith("_") or name in SKIP or not callable(f) or isinstance(f, type) or getattr(f, "__module__", "") != vh.__name__:
            continue
        kept[name] = f

        def inner(*a, _f=f, **k):
            count[0] += 1
            return _f(*a, **k)
        setattr(vh, name, inner)
    try:
        leg.run(1)
    finally:
        for name, f in kept.items():
            setattr(vh, name, f)
    return count[0]


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters())) and all(torch.equal(p, q) for p, q in zip(a.buffers(), b.buffers()))


def summary(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3)}


def steps_mode():
    for name in args.configs.split(","):
        cfg, precision, which = CONFIGS[name]
        for b in (int(v) for v in args.batches.split(",")):
            pool = batches(b)
            me = bench.build_net(cfg, HW, dev).train()
            legs = {"eager": Leg(eager_leg(me, precision, optimiser(me, which)), pool)}
            if not args.eager_only:
                mg = bench.build_net(cfg, HW, dev).train()
                legs["graph"] = Leg(graphed_leg(mg, precision, optimiser(mg, which)), pool)
            for leg in legs.values():
                leg.run(3)                                               # eager warm-up; the graphed leg: warm, capture, one replay
            times = {k: [] for k in legs}
            for rep in range(args.repeats):
                row = {"tree": tag, "config": name, "B": b, "rep": rep}
                for k, leg in legs.items():
                    times[k].append(leg.timed(args.steps))
                    row[k + "_ms"] = round(times[k][-1], 3)
                for k, leg in legs.items():
                    row[k + "_calls"] = wrapper_calls(leg)
                if "graph" in legs:
                    row["path"] = legs["graph"].fn.graphed.path
                    row["equal"] = bool(same(me, mg) and torch.equal(legs["eager"].loss, legs["graph"].loss))
                print(json.dumps(row), flush=True)
            out = {"tree": tag, "config": name, "B": b, "summary": {k: summary(v) for k, v in times.items()}}
            if "graph" in legs:
                out["linear"] = args.linear
                out["stats"] = legs["graph"].fn.graphed.stats
                out["graph_median_below_eager_min"] = out["summary"]["graph"]["median"] < out["summary"]["eager"]["min"]
            print(json.dumps(out), flush=True)
            del legs, me, pool
            if not args.eager_only:
                del mg
            torch.cuda.empty_cache()


def sgd_mode():
    """HRNet-W32's optimiser step alone: one vatl_sgd_step launch per tensor against one vatl_sgd_step_multi launch per group."""
    m = bench.build_net(bench.HRNET_W32, HW, dev).train()
    params = [p for p in m.parameters() if p.requires_grad]
    g = torch.Generator(device=dev); g.manual_seed(2)
    for p in params:
        p.grad = torch.rand(p.shape, device=dev, generator=g) * 1e-3
    opt = O.SGD(params, lr=2.5e-4, momentum=0.9, weight_decay=5e-4)
    multi = O.SGD._multi
    times = {"per_tensor": [], "multi": []}

    def timed(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6
    for warm in (True, False):
        for rep in range(1 if warm else args.repeats):
            row = {"tensors": len(params), "elements": sum(p.numel() for p in params), "rep": rep}
            for k in times:
                O.SGD._multi = None if k == "per_tensor" else staticmethod(multi)
                t = timed(3 if warm else args.steps)
                if not warm:
                    times[k].append(t)
                    row[k + "_us"] = round(t, 1)
            if not warm:
                print(json.dumps(row), flush=True)
    O.SGD._multi = staticmethod(multi)
    s = {k: summary(v) for k, v in times.items()}
    print(json.dumps({"sgd_step_us": s, "multi_median_below_per_tensor_min": s["multi"]["median"] < s["per_tensor"]["min"]}), flush=True)


if __name__ == "__main__":
    sgd_mode() if args.sgd else steps_mode()
