"""Inputs of the optimiser bit fixture (tests/golden/optim_bits.npz): what tools/make_optim_bits.py records and
tests/test_gpu_optim.py replays.  One tensor per optimiser kind, N = 1027 elements — 1024 that take the float4 body's arithmetic and
a tail of 3 — stepped STEPS = 3 times (SGD takes both of its forms), weight decay non-zero everywhere, a few gradients exactly 0.
Inputs are regenerated from the seeds, never stored."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_bits.npz")
N, STEPS = 1027, 3
ZERO_GRADS = (0, 5, 1023, 1024, 1026)              # body and tail elements

# kind -> (seed, state buffers in the calls' order, hyper-parameters as the vatl_hip wrappers name them)
CASES = {
    "adamw": (101, ("exp_avg", "exp_avg_sq"), dict(lr=2.5e-3, weight_decay=0.7, betas=(0.9, 0.999), eps=1e-8)),
    "adam": (102, ("exp_avg", "exp_avg_sq"), dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)),
    "sgd": (103, ("momentum_buffer",), dict(lr=2.5e-4, momentum=0.9, weight_decay=5e-4)),
    "rmsprop": (104, ("square_avg",), dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=5e-4)),
}


def inputs(kind):
    """-> (p, [g of step 1, 2, 3]) as float32 numpy arrays; the state buffers start at zero."""
    r = np.random.RandomState(CASES[kind][0])
    p = r.standard_normal(N).astype(np.float32)
    gs = [r.standard_normal(N).astype(np.float32) for _ in range(STEPS)]
    for g in gs:
        g[list(ZERO_GRADS)] = 0.0
    return p, gs


def run(vh, kind, p, gs, bufs, multi=False):
    """STEPS steps on the device tensors p / bufs in place, through the per-tensor wrapper or the multi one (a list of one tensor)."""
    fn = getattr(vh, kind + ("_step_multi" if multi else "_step"))
    for step, g in enumerate(gs, 1):
        tensors = [[t] for t in (p, g, *bufs)] if multi else [p, g, *bufs]
        fn(*tensors, *(() if kind == "rmsprop" else (step,)), **CASES[kind][2])


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)
