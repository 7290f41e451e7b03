#!/usr/bin/env python3
"""Step and epoch times of the WholeBodyAE pre-training path on one MI355X (profiles/ae_pretrain_notes.md).

    python tools/ae_pretrain_bench.py [--rows 10000] [--reps 100] [--epoch-rows 200000] [--out FILE]

HIP events around each warm step, median of ``--reps`` (>= 50), at the pre-training batch (10 000 x 42, z = 5):
  fused           one ``vatl_ae_train_step_large`` call (forward, MSELoss, backward, AdamW)
  autograd        ``WholeBodyAE.forward`` + ``nn.MSELoss`` + ``loss.backward()`` (``vatl_ae_forward`` + ``vatl_ae_backward``)
  autograd_adamw  the same followed by ``torch.optim.AdamW.step()`` on the sixteen tensors: the unchanged script's step
  eager           the yardstick: a plain ``nn.Sequential`` of the same topology in torch eager on the same GPU, forward + loss + backward
  eager_adamw     ... followed by ``torch.optim.AdamW.step()``: how the reference executes a step
and, by the host clock around work that ends in a device read-back:
  trainer_epoch   one epoch of ``pretrain_autoencoder`` on ``--epoch-rows`` synthetic rows (train) and a quarter as many (validation)
  loader_epoch    what the unchanged script spends on the host alone to collate the same rows through ``DataLoader`` (batches of
                  10 000 one-row tensors, shuffle), in-process and with 16 workers
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


def eager_net(d, z):
    dims = (d, 24, 12, 7, z, 7, 12, 24, d)
    layers = []
    for i in range(8):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i == 7:
            layers.append(nn.Sigmoid())
        elif i != 3:
            layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_us": statistics.median(ms) * 1e3, "min_us": min(ms) * 1e3, "p90_us": sorted(ms)[int(0.9 * (len(ms) - 1))] * 1e3}


class Rows(torch.utils.data.Dataset):
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return torch.tensor(self.rows[i], dtype=torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=42)
    ap.add_argument("--z", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--epoch-rows", type=int, default=200000)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ae_pretrain_bench needs an MI355X: a CPU run measures nothing")
    if a.reps < 50:
        raise SystemExit("--reps must be at least 50")
    import vatl_hip as vh
    from active_learning.Whole_body_AE import WholeBodyAE
    from active_learning.Whole_body_AE.pretrain import pretrain_autoencoder
    dev = torch.device("cuda:0")
    d, z, n = a.dim, a.z, a.rows
    torch.manual_seed(0)
    x = torch.rand(n, d, device=dev)
    crit = nn.MSELoss()
    res = {"rows": n, "dim": d, "z": z, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    ae = WholeBodyAE(z_dim=z, input_dim=d).to(dev).train()
    flat = vh.pack_ae(ae.state_dict(), dev).clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    ws, loss = vh.ae_grad_workspace(n, d, z, dev), torch.zeros(1, device=dev)
    step = [0]

    def fused():
        step[0] += 1
        vh.ae_train_step_large(flat, m, v, x, d, z, step[0], 1e-3, workspace=ws, loss=loss)

    res["fused"] = timed(fused, a.reps)

    opt = torch.optim.AdamW(ae.parameters(), lr=1e-3)

    def autograd(with_opt):
        def fn():
            l = crit(ae(x), x)
            opt.zero_grad()
            l.backward()
            if with_opt:
                opt.step()
        return fn

    res["autograd"] = timed(autograd(False), a.reps)
    res["autograd_adamw"] = timed(autograd(True), a.reps)

    net = eager_net(d, z).to(dev).train()
    eopt = torch.optim.AdamW(net.parameters(), lr=1e-3)

    def eager(with_opt):
        def fn():
            l = crit(net(x), x)
            eopt.zero_grad()
            l.backward()
            if with_opt:
                eopt.step()
        return fn

    res["eager"] = timed(eager(False), a.reps)
    res["eager_adamw"] = timed(eager(True), a.reps)

    rows = torch.rand(a.epoch_rows, d)
    valid = torch.rand(max(1, a.epoch_rows // 4), d)
    pretrain_autoencoder(rows[:20000], valid[:8000], z, epochs=1)                          # warm: code objects, pinned staging, workspaces
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pretrain_autoencoder(rows, valid, z, epochs=a.epochs)
    torch.cuda.synchronize()
    res["trainer_epoch"] = {"rows": a.epoch_rows, "valid_rows": len(valid), "epochs": a.epochs, "ms_per_epoch_incl_upload": (time.perf_counter() - t0) * 1e3 / a.epochs}

    data = Rows(rows.numpy())
    for workers in (0, 16):
        loader = torch.utils.data.DataLoader(data, batch_size=10000, shuffle=True, num_workers=workers, pin_memory=True)
        t0 = time.perf_counter()
        batches = sum(1 for _ in loader)
        res[f"loader_epoch_workers{workers}"] = {"rows": a.epoch_rows, "batches": batches, "ms": (time.perf_counter() - t0) * 1e3}

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
