#!/usr/bin/env python3
"""Headline benchmark: frames/s of pose inference + uncertainty scoring.

Workload (BASELINE.json configs[1]): SimpleBaseline
ResNet-50, 256x192 crops, 17 key-points, a 1024-frame synthetic video per GPU
(4 tracks x 256 consecutive frames, id-sorted), batches of 256:
    one "step" = backbone forward (one per frame, de-duplicated neighbours)
               + arg-max decode + local-peak mean + THC-L1 over the whole video.
Inputs are resident in HBM before the timed region.  Random-init weights of the
named architecture, synthetic crops (no dataset / checkpoint on the box).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full [--no-extra] [--no-cpu-baseline]]
N > 1: one rank per GPU over RCCL.  Under torch.distributed.run the ranks are given (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_*); run bare, `--gpus N` starts the N ranks itself as fresh child processes before anything
touches a GPU (never an exec of this process) and relays rank 0's line.  Frames shard across ranks (weak scaling:
1024 frames per rank), per-item results are all-gathered; there is no other exchange on this path.

`--dump-outputs DIR` writes, after the timed steps, what rank 0's last timed step returned (key-points, arg-max indices, HP,
pose score, local-peak mean, THC and a fixed, seeded sample of the heat-maps) as DIR/<name>.npy in float32 / float64, so that
two builds can be compared output for output on the same seeded inputs.

Prints ONE JSON line on rank 0 (contract: tests/test_gpu_bench.py) with the headline: `metric`, `value` (frames/s over all ranks),
`unit`, `higher_is_better`, `dtype`, `ms_per_step`.  A plain run does only that: set-up, warm-up, the timed steps, `--dump-outputs`, the line.
`--full` runs the same set-up, warm-up and timed steps and then adds what takes runs of its own: `roofline` (conv implicit-GEMM launches of one
more step timed with HIP events, the shader clock sampled over the timed steps), at N = 1 `cpu_baseline` (the oracle restatement timed on the
host cores, bounded sample; `--no-cpu-baseline` skips it), and `extra` (`--no-extra` skips it): the headline variants and the other
BASELINE.json configurations measured in the same run — configs[2] SimpleBaseline-R50 fine-tune step (fwd + bwd + AdamW, B = 120 per GPU,
gradient arena all-reduced over RCCL at N > 1), configs[3] HRNet-W32 inference + THC + WPU on a 1024-frame shard with its halo, configs[4]
FastPose-R152 384x288 fine-tune step (B = 32 per GPU, 301 MB gradient all-reduce at N > 1).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "vatl4pose-wacv2024_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)



def granted_cpus():
    """CPUs this process may USE: the affinity mask, cut down to the cgroup's CPU-time quota (the GPU boxes show 256 logical CPUs to a container that is
    granted 16: /sys/fs/cgroup/cpu.max "1600000 100000")."""
    visible = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    return (max(1, min(visible, int(quota + 0.5))) if quota else visible), visible, quota


# Host thread pools sized to the GRANTED CPUs, before torch / numpy create them (setdefault: an explicit setting of the caller wins).  Left at their
# default — one worker per VISIBLE core, 256 on the GPU boxes — a single parallel region of torch's intra-op pool or of numpy's BLAS spins 256 threads
# against a 16-CPU quota; the kernel then throttles the whole process for the rest of the 100 ms period, main thread and HIP runtime threads included
# (r06: single 85 - 109 ms rounds among 71 ms ones in `extra.product_entry_points` with no collector pass in them).
for _v in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
    os.environ.setdefault(_v, str(granted_cpus()[0]))

import torch  # noqa: E402

FRAMES = 1024
TRACKS = 4
BATCH = 1024                     # the reference's AL config evaluates 1080 crops per call (al_simple_posetrack.yaml:73)
GFLOP_PER_CROP = 10.853          # SimplePose-R50 256x192 forward, conv+deconv MACs x 2
PEAK_FP32_MFMA = 157.3           # TFLOP/s, v_mfma_f32_32x32x2_f32 (MI355X_MICROARCH.md)


NOMINAL_SCLK_MHZ = 2400.0        # the shader clock the 157.3 TFLOP/s figure is quoted at (256 CUs x 256 fp32 MFMA FLOP / cycle / CU x 2.4 GHz)


class ClockSampler:
    """Shader clock and socket power of ONE GPU while a region runs: a plain host thread reads the amdgpu hwmon files
    (`freq1_input` = sclk in Hz, `power1_input` / `power1_average` in uW) every `period` seconds.  No torch call inside the thread — a
    torch CPU op here would start torch's intra-op pool, whose spinning workers stall the HIP runtime's launch threads
    (profiles/r05_hip_stalls.txt).  The card is found by the PCI address of the torch device; without a match (or without readable
    files: a container that hides sysfs) every figure is None and the bench line says so."""

    def __init__(self, dev_index: int, period: float = 0.01):
        self.period, self.samples, self._stop, self._thread = period, [], threading.Event(), None
        self.hwmon, self.why = None, None
        try:
            pr = torch.cuda.get_device_properties(dev_index)
            want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
        except Exception as e:                                             # noqa: BLE001 (older torch: no PCI fields)
            want, self.why = None, f"no PCI address from torch ({e})"
        base = "/sys/class/drm"
        cands = []
        try:
            for card in sorted(os.listdir(base)):
                if not card.startswith("card") or "-" in card:
                    continue
                devdir = os.path.join(base, card, "device")
                pci = os.path.basename(os.path.realpath(devdir))
                hw = os.path.join(devdir, "hwmon")
                for h in (sorted(os.listdir(hw)) if os.path.isdir(hw) else []):
                    if os.access(os.path.join(hw, h, "freq1_input"), os.R_OK):
                        cands.append((pci, os.path.join(hw, h)))
        except OSError as e:
            self.why = f"sysfs not readable ({e})"
        for pci, h in cands:
            if want and pci.lower().startswith(want):
                self.hwmon, self.pci = h, pci
        if self.hwmon is None and len(cands) == 1:                        # one card visible: it is ours
            self.pci, self.hwmon = cands[0]
        if self.hwmon is None and self.why is None:
            self.why = f"no hwmon directory for PCI {want} among {[c[0] for c in cands]}"

    def _read(self, name):
        try:
            with open(os.path.join(self.hwmon, name)) as f:
                return int(f.read().strip())
        except (OSError, ValueError):
            return None

    def _run(self):
        while not self._stop.is_set():
            f = self._read("freq1_input")
            pw = self._read("power1_input")
            if pw is None:
                pw = self._read("power1_average")
            if f is not None:
                self.samples.append((time.perf_counter(), f / 1e6, None if pw is None else pw / 1e6))
            self._stop.wait(self.period)

    def __enter__(self):
        if self.hwmon is not None:
            self._thread = threading.Thread(target=self._run, name="vatl-sclk", daemon=True)
            self._thread.start()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.t1 = time.perf_counter()
        self._stop.set()
        if self._thread is not None:
            self._thread.join()
        return False

    def summary(self, t0=None, t1=None):
        """Clock statistics of the samples taken inside [t0, t1] (default: the whole region), skipping the first 10 % (ramp-up)."""
        t0, t1 = (self.t0 if t0 is None else t0), (self.t1 if t1 is None else t1)
        t0 = t0 + 0.1 * (t1 - t0)
        mhz = sorted(m for t, m, _ in self.samples if t0 <= t <= t1)
        pw = [w for t, _, w in self.samples if t0 <= t <= t1 and w is not None]
        if not mhz:
            return {"sclk_mhz_mean": None, "sclk_samples": 0, "sclk_source": self.why or "no sample inside the timed region"}
        q = lambda x: mhz[min(len(mhz) - 1, int(x * len(mhz)))]
        return {"sclk_mhz_mean": round(sum(mhz) / len(mhz), 1), "sclk_mhz_min": round(mhz[0], 1), "sclk_mhz_median": round(q(0.5), 1), "sclk_mhz_max": round(mhz[-1], 1),
                "sclk_samples": len(mhz), "power_w_mean": round(sum(pw) / len(pw), 1) if pw else None,
                "sclk_source": f"{self.hwmon}/freq1_input (PCI {self.pci}), sampled every {self.period * 1e3:.0f} ms by a host thread over the timed region of the headline"}


def build_model(dev):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    cfg = edict({"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50})
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]})
    torch.manual_seed(166)
    m = builder.build_sppe(cfg, preset_cfg=preset)
    with torch.no_grad():                              # random running stats so BN folding is exercised
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    return m.to(dev).eval()


def make_video(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.rand((FRAMES, 3, 256, 192), device=dev, generator=g)
    x -= torch.tensor([0.406, 0.457, 0.480], device=dev).view(1, 3, 1, 1)
    w = 60 + 180 * torch.rand(FRAMES, device=dev, generator=g)
    bbox = torch.stack([torch.full_like(w, 100.0), torch.full_like(w, 50.0), 100 + w, 50 + w * 4 / 3], 1).contiguous()
    pos = torch.arange(FRAMES, device=dev) % (FRAMES // TRACKS)
    return x, bbox, (pos != 0).to(torch.uint8), (pos != FRAMES // TRACKS - 1).to(torch.uint8)


def one_step(model, x, bbox, is_prev, is_next, hm_buf, batch=None):
    from active_learning.scoring import score_batch
    from alphapose.models import hip_engine
    batch = batch or BATCH
    with torch.no_grad():
        for i in range(0, FRAMES, batch):
            hip_engine.forward_into(model, x[i:i + batch], hm_buf[i:i + batch])
        return score_batch(hm_buf, bbox, is_prev, is_next, thc_norm="L1")


def headline_variants(model, x, bbox, is_prev, is_next, hm_buf, steps=3):
    """Beside the headline (one 1024-crop launch sequence per video, one forward per frame): the same step in batches of 256 (SURVEY.md
    §8d item 2's sketch), and the §8d item 3 pair — the reference-faithful evaluation that forwards the prev / current / next crops of
    every item (ActiveLearning.py:277, 294, 296) against the de-duplicated stream, THC compared bit for bit."""
    import vatl_hip as vh
    from active_learning.scoring import score_batch
    from alphapose.models import hip_engine

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    out = {}
    d256 = timed(lambda: one_step(model, x, bbox, is_prev, is_next, hm_buf, batch=256))
    out["batch256_frames_per_s"] = round(FRAMES / d256, 1)
    out["batch256_ms_per_step"] = round(d256 * 1e3, 3)
    a = one_step(model, x, bbox, is_prev, is_next, hm_buf)
    thc_dedup = a.thc.clone()
    d1 = timed(lambda: one_step(model, x, bbox, is_prev, is_next, hm_buf))
    prev_x = torch.cat([torch.zeros_like(x[:1]), x[:-1]]) * is_prev.view(-1, 1, 1, 1)
    next_x = torch.cat([x[1:], torch.zeros_like(x[:1])]) * is_next.view(-1, 1, 1, 1)
    hp, hn = torch.empty_like(hm_buf), torch.empty_like(hm_buf)

    def faithful():                                   # three forwards per item, THC from explicit neighbour heat-maps
        with torch.no_grad():
            hip_engine.forward_into(model, x, hm_buf)
            hip_engine.forward_into(model, prev_x, hp)
            hip_engine.forward_into(model, next_x, hn)
            s = score_batch(hm_buf, bbox, is_prev, is_next, thc_norm=None)
            tp, tn = vh.thc_pairs(hm_buf, hp, "L1"), vh.thc_pairs(hm_buf, hn, "L1")
            one = (is_prev ^ is_next).float()
            s.thc = (tp * is_prev + tn * is_next) * (1 + one)
            return s
    b = faithful()
    torch.cuda.synchronize()
    out["thc_bit_identical"] = bool(torch.equal(thc_dedup, b.thc))
    d3 = timed(faithful)
    out["dedup_frames_per_s"] = round(FRAMES / d1, 1)
    out["faithful_3fwd_frames_per_s"] = round(FRAMES / d3, 1)
    del prev_x, next_x, hp, hn
    torch.cuda.empty_cache()
    return out


def conv_roofline(model, x, bbox, is_prev, is_next, hm_buf):
    """Time every conv / deconv launch of one step with HIP events on the launch stream (torch's current stream) and relate the sum
    to (a) the MFMA FLOPs those launches really execute — counted by the library itself, tile padding included
    (vatl_flop_meter_begin / _end) — and (b) the algorithmic (direct-sum) FLOPs of the step.  `frac` is (a): the fraction of the
    fp32 matrix pipe's peak that is busy; it cannot exceed 1.  (b) is `algorithmic_frac`: 16 of the step's launches are Winograd
    kernels that reach their direct-sum FLOPs with 2.25x fewer multiplies, so it can."""
    import vatl_hip as vh
    events, wino = [], []
    # every entry point of the step that launches MFMA work (the library meters their FLOPs; a launch missing here would count FLOPs without time: checked below)
    timed_names = {"conv2d_fwd": 0, "deconv4x4s2_fwd": 0, "conv1x1_dual_fwd": 0, "conv3x3_winograd_fwd": 9, "deconv4x4s2_winograd_fwd": 4,
                   "stem_pool_fwd": 0,               # the fused stem: conv1 + bn1 + relu + maxpool in one launch — its pooling is inside the timed launch
                   "bottleneck_chain_fwd": 0,        # conv3 + skip of one bottleneck and conv1 of the next in one launch
                   "conv1x1_rows_fwd": 0,            # K = 128 1x1 layers as a row-streaming GEMM
                   "conv3x3_winograd_c32_fwd": 9,    # 32 -> 32 channel 3x3 layers (HRNet): wave-private Winograd
                   "conv3x3_winograd_f4_fwd": 9}     # 3x3 layers on grids of whole 4x4 tiles: Winograd F(4x4,3x3)
    originals = {n: getattr(vh, n) for n in timed_names}

    inside = [0]                                           # metered launches made inside timed entry-point calls

    def wrap(fn, is_wino=0):
        def inner(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before = vh.flop_meter.launches_now()
            e0.record()
            r = fn(*a, **k)
            e1.record()
            inside[0] += vh.flop_meter.launches_now() - before
            events.append((e0, e1))
            if is_wino:                                    # direct-sum FLOPs of this launch: 2 * output elements * taps * Cin (9 / 4 taps)
                wino.append((e0, e1, 2.0 * r.numel() * is_wino * a[0].shape[-1]))
            return r
        return inner
    for n, taps in timed_names.items():
        setattr(vh, n, wrap(originals[n], taps))
    try:
        with vh.flop_meter() as fm:
            one_step(model, x, bbox, is_prev, is_next, hm_buf)
        torch.cuda.synchronize()
    finally:
        for n, fn in originals.items():
            setattr(vh, n, fn)
    # One entry-point call may make several metered launches (the persistent Winograd route + the plain kernel for the images that do not fill a
    # period; split-K): what must hold is that every metered launch happened INSIDE a timed call — FLOPs without time would inflate `frac`.
    metered = fm.direct_launches + fm.winograd_launches
    if metered != inside[0] or metered < len(events):
        raise RuntimeError(f"conv_roofline: {metered} metered MFMA launches, {inside[0]} of them inside the {len(events)} timed entry-point calls — "
                           "an entry point is missing from timed_names")
    ms = sum(a.elapsed_time(b) for a, b in events)
    flops = GFLOP_PER_CROP * 1e9 * x.shape[0]
    algorithmic = flops / (ms * 1e-3) / 1e12
    executed = fm.total                                    # what the matrix pipe multiplies: padded tiles, 16 / 36 of the direct sum on the Winograd launches
    achieved = executed / (ms * 1e-3) / 1e12
    wino_flops = sum(f for _, _, f in wino)
    wino_ms = sum(a.elapsed_time(b) for a, b, _ in wino)
    traffic, traffic_source = None, None               # HBM bytes of the same launches, from the committed PMC passes
    try:
        pmcs = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc_summary.json"))
        with open(os.path.join(ROOT, "profiles", pmcs[-1])) as f:
            traffic = json.load(f)["conv_igemm"]["hbm_bytes_per_step"]
        traffic_source = "profiles/" + pmcs[-1]
    except (OSError, IndexError, KeyError, ValueError):
        pass
    return {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_FP32_MFMA, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_FP32_MFMA, 4), "traffic": (traffic / len(events)) if traffic else None,
            "metered_launches": metered, "timed_calls": len(events), "kernel": "stem_pool_kernel + conv_igemm_kernel + gemm1x1_persistent2_kernel + conv1x1_rows_kernel / conv1x1_rows256_kernel + bottleneck_chain_kernel + winograd_kernel / winograd_persist_kernel (all conv/deconv launches of one step; the stem launch includes bn1 + relu + maxpool; 4 launches fuse a projection shortcut with the block's last conv, 1 chains a block's last conv with the next block's first; of the 13 3x3 stride-1 layers the 11 on grids of whole 4x4 tiles run as Winograd F(4x4,3x3) (winograd_f4_kernel), the 2 at 8x6 as F(2x2,3x3), the 3 transposed convs as F(3x3,2x2) on their four phases)", "launches": len(events),
            # `achieved` / `frac`: MFMA FLOPs the launches EXECUTE (counted per launch by libvatl_hip.so: 2 x padded M x padded N x padded K; the
            # Winograd launches their 16 transform-domain GEMMs) / event-timed duration / peak = how busy the matrix pipe is.
            # `algorithmic_*`: the step's direct-sum FLOPs (10.853 GFLOP x frames) over the same time; the Winograd launches deliver
            # theirs with 2.25x fewer multiplies, so this ratio may exceed 1 — it is a throughput figure, not a roofline fraction.
            "executed_flops_per_step": executed, "executed_direct_flops": fm.direct, "executed_winograd_flops": fm.winograd,
            "algorithmic_achieved": round(algorithmic, 2), "algorithmic_frac": round(algorithmic / PEAK_FP32_MFMA, 4),
            "winograd": {"launches": len(wino), "ms": round(wino_ms, 3), "algorithmic_tflops": round(wino_flops / (wino_ms * 1e-3) / 1e12, 2) if wino_ms else None,
                         "executed_tflops": round(fm.winograd / (wino_ms * 1e-3) / 1e12, 2) if wino_ms else None,
                         "executed_frac": round(fm.winograd / (wino_ms * 1e-3) / 1e12 / PEAK_FP32_MFMA, 4) if wino_ms else None},
            "implicit_gemm": {"launches": len(events) - len(wino), "ms": round(ms - wino_ms, 3),
                              "executed_tflops": round(fm.direct / ((ms - wino_ms) * 1e-3) / 1e12, 2),
                              "executed_frac": round(fm.direct / ((ms - wino_ms) * 1e-3) / 1e12 / PEAK_FP32_MFMA, 4)},
            "avg_launch_us": round(ms * 1e3 / len(events), 2), "flops_per_step": flops,
            # the step's conv launches have different shapes: `achieved` is sum(flops) / sum(duration); per-launch averages for reference
            "flops_per_launch": executed / len(events), "traffic_per_step": traffic, "traffic_source": traffic_source,
            "traffic_note": "`traffic` = HBM bytes per launch (average over the step's conv launches, like `achieved`); source: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (FETCH_SIZE x2 on gfx950) around this same command (tools/profile_round.sh), summed over the conv launches of one step — read from `traffic_source`, the newest committed summary: the counters cannot be sampled from inside the process, so this field does not move with the run"}


def cpu_baseline():
    """The oracle (CPU restatement of the reference graph + scorers) on the host cores, bounded sample: 32 crops forward + decode / local-peak /
    THC of 32 items.  The thread count is calibrated AT the measured batch (one warm-up + one timed forward of the 32 crops per candidate,
    candidates up to every core the process may use), the winner and the all-cores count are timed three times each (median), the faster is reported and the all-cores figure beside it."""
    import numpy as np
    from oracle import nets, scorers, synth
    m = nets.SimplePoseRef(50).eval()
    n = 32
    x = torch.from_numpy(synth.crops(n, seed=1))
    # The cores this process may actually USE: the GPU boxes show 256 logical CPUs to a container whose cgroup grants 16 CPUs of time
    # (cpu.max "1600000 100000") — 256 runnable threads against that quota are throttled to a crawl (measured: 36.8 s per 32-crop forward
    # against 0.9 s with 16 threads).  "All cores" therefore means all GRANTED cores.
    avail, visible, quota = granted_cpus()
    cands = sorted({c for c in (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512) if c < avail} | {avail})
    calib, budget = {}, time.perf_counter() + 45.0
    with torch.no_grad():
        for th in reversed(cands):                                 # all granted cores first: that figure is reported whatever wins
            torch.set_num_threads(th)
            m(x)
            t0 = time.perf_counter()
            m(x)
            calib[th] = time.perf_counter() - t0
            if time.perf_counter() > budget or calib[th] > 2.5 * min(calib.values()):
                break                                              # out of time, or far past the optimum (fewer threads only get slower from here)

    def median_fwd(th):                                            # one warm-up + median of 3 timed forwards at `th` threads
        torch.set_num_threads(th)
        ts = []
        with torch.no_grad():
            m(x)
            for _ in range(3):
                t0 = time.perf_counter()
                hm = m(x).numpy()
                ts.append(time.perf_counter() - t0)
        return sorted(ts)[1], hm

    # The calibration timed each candidate once: the winner and the all-cores count are re-timed the same way (median of 3), and the faster of the two
    # is reported, so the all-cores figure beside it is never a luckier single sample of the same configuration.
    cores = min(calib, key=calib.get)
    fwd, hm = median_fwd(cores)
    fwd_all = fwd
    if cores != avail:                                             # (avail is always a candidate: the loop starts there)
        fwd_all, hm_all = median_fwd(avail)
        if fwd_all < fwd:
            cores, fwd, hm = avail, fwd_all, hm_all
    bb = synth.bboxes(n)
    t0 = time.perf_counter()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(n):
            scorers.decode_heatmaps(hm[i], bb[i])
            scorers.localpeak_mean(hm[i])
            if i:
                scorers.thc_pair(hm[i], hm[i - 1])
    post = time.perf_counter() - t0
    cpu_model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"value": round(n / (fwd + post), 2), "unit": "frames/s", "cores": cores, "cores_available": avail, "cores_visible": visible, "cgroup_cpu_quota": quota, "cpu_model": cpu_model, "kind": "port",
            "sample": f"{n} crops: SimplePose-R50 forward (torch CPU fp32, {cores} threads = the fastest of {sorted(calib)} timed at this batch, median of 3) + numpy decode/local-peak/THC",
            "forward_s": round(fwd, 3), "scoring_s": round(post, 3),
            "all_cores": {"cores": avail, "value": round(n / (fwd_all + post), 2), "forward_s": round(fwd_all, 3)},
            "calibration_forward_s": {str(k): round(v, 3) for k, v in sorted(calib.items())}}


# ---------------------------------------------------------------------------------------------------------------------
# the other BASELINE.json configurations (reported under "extra" of the same JSON line)
# ---------------------------------------------------------------------------------------------------------------------

HRNET_W32 = {"TYPE": "PoseHighResolutionNet", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 50, "FINAL_CONV_KERNEL": 1, "PRETRAINED_LAYERS": ["*"],
             "STAGE2": {"NUM_MODULES": 1, "NUM_BRANCHES": 2, "NUM_BLOCKS": [4, 4], "NUM_CHANNELS": [32, 64], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"},
             "STAGE3": {"NUM_MODULES": 4, "NUM_BRANCHES": 3, "NUM_BLOCKS": [4, 4, 4], "NUM_CHANNELS": [32, 64, 128], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"},
             "STAGE4": {"NUM_MODULES": 3, "NUM_BRANCHES": 4, "NUM_BLOCKS": [4, 4, 4, 4], "NUM_CHANNELS": [32, 64, 128, 256], "BLOCK": "BASIC", "FUSE_METHOD": "SUM"}}
SIMPLE_R50 = {"TYPE": "SimplePose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_LAYERS": 50}
FAST_R152 = {"TYPE": "FastPose", "PRETRAINED": "", "TRY_LOAD": "", "NUM_LAYERS": 152}
GFLOP_FWD = {"simplepose_r50": 10.853, "hrnet_w32": 15.290, "fastpose_r152_384": 59.192}      # per crop, SURVEY.md §8d


def build_net(cfg, hw, dev):
    from alphapose.models import builder
    from alphapose.utils.config import edict
    preset = edict({"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": list(hw), "HEATMAP_SIZE": [hw[0] // 4, hw[1] // 4]})
    torch.manual_seed(166)
    m = builder.build_sppe(edict(cfg), preset_cfg=preset)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
    return m.to(dev)


def _timed(fn, steps, warmup, dist_on):
    """Barrier + synchronize on both sides, max over ranks (same bracket as the headline)."""
    import torch.distributed as td
    for _ in range(warmup):
        fn()
    if dist_on:
        td.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    if dist_on:
        td.barrier()
    dt = time.perf_counter() - t0
    if dist_on:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        dt = float(t.item())
    return dt / steps


def finetune_step_fn(m, opt, x, labels, masks, world, reduce=True):
    """One data-parallel fine-tune step as ActiveLearning.retrain_model runs it: train-mode forward, fused masked-MSE loss +
    gradient (scaled by this rank's share of the global mini-batch), backward into the flat gradient arena whose finished
    buckets are all-reduced over RCCL while the backward is still running, AdamW on the arena slices."""
    import vatl_hip as vh
    from alphapose.models import hip_train
    tr, arena = hip_train.trainer_for(m), hip_train.arena_for(m)

    def step():
        with torch.no_grad():
            out = tr.forward(x)
            loss, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
            if world > 1:
                dout.mul_(1.0 / world)
            arena.begin()
            if not reduce:                                   # the same step with its collectives switched off (overlap accounting)
                arena._live = False
            tr.backward(dout, arena=arena, overlap=True)
            arena.finish()
            arena.attach()
        opt.step()
        return loss
    return step, arena


def _allreduce_alone_ms(arena, dist_on):
    """The gradient all-reduce by itself (not overlapped): what the step would pay if nothing hid it."""
    if not dist_on:
        return None
    import torch.distributed as td
    for _ in range(2):
        td.all_reduce(arena.flat)
    torch.cuda.synchronize()
    td.barrier()
    t0 = time.perf_counter()
    for _ in range(5):
        td.all_reduce(arena.flat)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / 5 * 1e3, 3)


def extra_finetune(dev, name, cfg, hw, batch, gflop_fwd, groups, world, dist_on, steps=8, warmup=4):
    # (warm-up 4: the first step records the weight re-pack plan and creates the optimizer state, the next ones let the caching allocator settle
    # under the two-stream pattern — with two warm-up steps one run in two still had a ~20 ms allocation step among its timed ones)
    from active_learning.optim import AdamW
    m = build_net(cfg, hw, dev).train()
    lr = 2.5e-4                                              # al_simple_posetrack.yaml:62-69: lr x{10, 1, 5}, weight decay 0.7
    opt = AdamW(params=[{"params": getattr(m, a).parameters(), "lr": lr * f} for a, f in groups], weight_decay=0.7)
    g = torch.Generator(device=dev)
    g.manual_seed(166 + int(os.environ.get("RANK", "0")))
    x = torch.rand((batch, 3, hw[0], hw[1]), device=dev, generator=g) - 0.45
    labels = torch.rand((batch, 17, hw[0] // 4, hw[1] // 4), device=dev, generator=g) * 0.1
    masks = (torch.rand((batch, 17, 1, 1), device=dev, generator=g) > 0.2).float()
    step, arena = finetune_step_fn(m, opt, x, labels, masks, world)
    dt = _timed(step, steps, warmup, dist_on)
    buckets = arena.launches if dist_on else 0
    alone = _allreduce_alone_ms(arena, dist_on)
    local_ms = hidden = None
    if dist_on:
        # the same step with no gradient exchange (what this rank would take alone) -> how much of the all-reduce the overlap hides:
        # overlap_hidden_frac = 1 - (step_N - step_local) / allreduce_alone   (1 = fully hidden, 0 = fully exposed)
        local_step, _ = finetune_step_fn(m, opt, x, labels, masks, world, reduce=False)
        local_ms = round(_timed(local_step, steps, 1, dist_on) * 1e3, 3)
        if alone:
            hidden = round(max(0.0, min(1.0, 1.0 - (dt * 1e3 - local_ms) / alone)), 4)
    tf = 3 * gflop_fwd * 1e9 * batch / dt / 1e12              # fwd + dgrad + wgrad of every conv, per GPU
    import vatl_hip as vh
    with vh.flop_meter() as fm:                              # one more (untimed) step: the MFMA FLOPs its launches execute, padding included
        step()
    torch.cuda.synchronize()
    ex = fm.total / dt / 1e12
    out = {"workload": name, "batch_per_gpu": batch, "ms_per_step": round(dt * 1e3, 3), "crops_per_s": round(batch * world / dt, 1),
           # executed_*: what the matrix pipe multiplies (library meter) / the WHOLE step time / peak — the roofline fraction of the step;
           # algorithmic_*: 3 x forward direct-sum FLOPs / the same time (the Winograd launches reach theirs with 2.25x fewer multiplies)
           "executed_tflops_per_gpu": round(ex, 2), "executed_frac": round(ex / PEAK_FP32_MFMA, 4),
           "executed_winograd_share": round(fm.winograd / fm.total, 4) if fm.total else None,
           "algorithmic_tflops_per_gpu": round(tf, 2), "algorithmic_frac": round(tf / PEAK_FP32_MFMA, 4),
           "grad_bytes": arena.total * 4, "allreduce_buckets": buckets, "allreduce_bucket_bytes": arena.bucket * 4,
           "allreduce_alone_ms": alone, "step_without_allreduce_ms": local_ms, "overlap_hidden_frac": hidden,
           "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    del m, opt, step, arena, x, labels, masks
    torch.cuda.empty_cache()
    return out


def extra_hrnet_shard(dev, world, rank, dist_on, steps=3, warmup=1):
    """configs[3]: HRNet-W32 inference + THC-L1 + WPU on this rank's 1024-frame shard of an id-sorted 1024 x N stream: interior
    shard edges recompute one halo frame (no heat-map exchange), the result rows are all-gathered."""
    import torch.distributed as td
    from active_learning.scoring import score_batch
    from active_learning.Whole_body_AE.AutoEncoder import WholeBodyAE
    from alphapose.models import hip_engine
    m = build_net(HRNET_W32, (256, 192), dev).eval()
    ae = WholeBodyAE(z_dim=4, kp_direct=False, input_dim=42).to(dev)
    flat = ae.packed()
    front, back = int(rank > 0), int(rank < world - 1)
    n = FRAMES + front + back
    g = torch.Generator(device=dev)
    g.manual_seed(1660 + rank)
    x = torch.rand((n, 3, 256, 192), device=dev, generator=g) - torch.tensor([0.406, 0.457, 0.480], device=dev).view(1, 3, 1, 1)
    w = 60 + 180 * torch.rand(n, device=dev, generator=g)
    bbox = torch.stack([torch.full_like(w, 100.0), torch.full_like(w, 50.0), 100 + w, 50 + w * 4 / 3], 1).contiguous()
    pos = (torch.arange(n, device=dev) - front) % (FRAMES // TRACKS)
    ip, inx = (pos != 0).to(torch.uint8), (pos != FRAMES // TRACKS - 1).to(torch.uint8)
    hm = torch.empty((n, 17, 64, 48), device=dev)
    backend_nccl = dist_on and td.get_backend() == "nccl"

    def run():
        with torch.no_grad():
            hip_engine.forward_into(m, x, hm)
            s = score_batch(hm, bbox, ip, inx, thc_norm="L1", ae_flat=flat, ae_dims=(42, 4))
            if dist_on:
                row = torch.cat([s.keypoints.reshape(n, -1), s.thc[:, None], s.wpu[:, None], s.localpeak[:, None]], 1)[front:n - back].contiguous()
                if not backend_nccl:
                    row = row.cpu()
                out = [torch.empty_like(row) for _ in range(world)]
                td.all_gather(out, row)
        return s

    dt = _timed(run, steps, warmup, dist_on)
    tf = GFLOP_FWD["hrnet_w32"] * 1e9 * n / dt / 1e12
    import vatl_hip as vh
    with vh.flop_meter() as fm:
        run()
    torch.cuda.synchronize()
    ex = fm.total / dt / 1e12
    out = {"workload": "HRNet-W32 256x192 inference + decode + local-peak + THC-L1 + WPU (AE 42-d, z=4), 1024-frame shard per GPU + halo",
           "frames_per_gpu": FRAMES, "halo_frames": front + back, "ms_per_pass": round(dt * 1e3, 3), "frames_per_s": round(FRAMES * world / dt, 1),
           # executed_*: MFMA FLOPs the launches execute (library meter, padding included) / whole pass time / peak; algorithmic_*: direct-sum
           # FLOPs over the same time — nearly every conv of the HRNet branches is a 3x3 on the Winograd route, so that ratio can exceed 1
           "executed_tflops_per_gpu": round(ex, 2), "executed_frac": round(ex / PEAK_FP32_MFMA, 4),
           "executed_winograd_share": round(fm.winograd / fm.total, 4) if fm.total else None,
           "algorithmic_tflops_per_gpu": round(tf, 2), "algorithmic_frac": round(tf / PEAK_FP32_MFMA, 4)}
    del m, x, hm
    torch.cuda.empty_cache()
    return out


def _synthetic_frame_video(n_frames, tracks, hw=(480, 640), seed=166, J=17):
    """Decoded uint8 RGB frames + one annotation per (track, frame) in the field layout the reference's loaders build (posetrack21.py:103-115):
    a person box drifting through the frame, joints inside it, ~15 % invisible; `id` orders the items track by track, frame by frame."""
    import numpy as np
    r = np.random.RandomState(seed)
    frames = [r.randint(0, 256, (hw[0], hw[1], 3), dtype=np.uint8) for _ in range(n_frames)]
    anns = []
    for t in range(tracks):
        x0, y0 = r.uniform(10, hw[1] * 0.4), r.uniform(5, hw[0] * 0.2)
        w, h = r.uniform(50, 110), r.uniform(110, 170)
        for f in range(n_frames):
            bx, by = x0 + 3.5 * f + r.uniform(-1, 1), y0 + 1.25 * f + r.uniform(-1, 1)
            j3 = np.zeros((J, 3, 2), np.float32)
            j3[:, 0, 0], j3[:, 1, 0] = r.uniform(bx, bx + w, J), r.uniform(by, by + h, J)
            vis = (r.random_sample(J) > 0.15).astype(np.float32)
            j3[:, 0, 1] = j3[:, 1, 1] = vis
            j3[:, :, 0] *= j3[:, :, 1]
            kp = np.stack([j3[:, 0, 0], j3[:, 1, 0], vis], 1).reshape(-1).astype(np.float32)
            anns.append({"bbox": (float(bx), float(by), float(bx + w), float(by + h)), "joints_3d": j3, "keypoint": kp.tolist(),
                         "id": t * 100000 + f, "ann_id": 500000 + t * 1000 + f, "img_id": 9000 + f, "track_id": f"v{t}", "frame": f})
    return frames, anns


def extra_product_entry_points(dev, items=1024, tracks=16, rounds=8):
    """The reference-shaped entry points themselves, wall clock in this process (verdict r04 item 5): `ActiveLearning.eval_and_query`
    (ActiveLearning.py:253-429) on 1024 decoded items — uint8 frames -> device crops (FrameVideo) -> SimpleBaseline-R50 in loader batches of 256 ->
    decode / THC / WPU / local-peak / OKS -> result records written -> query — and `ActiveLearning.retrain_model` (:651-686) over the same items
    (9 mini-batches of 120 with host-side augmentation parameters, device crops and targets, AdamW, the WPU auto-encoder refit).  Host work included:
    this is the figure a user of the drop-in sees; the headline above is the device-resident rate of the same kernels."""
    import tempfile
    import types
    import numpy as np
    from active_learning import ActiveLearning
    from alphapose.datasets import FrameVideo
    from alphapose.utils.config import edict
    frames, anns = _synthetic_frame_video(items // tracks, tracks)
    preset = {"IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48], "SIGMA": 2}
    ev = FrameVideo(frames, anns, train=False, get_prenext=True, PRESET=preset)
    tr = FrameVideo(frames, anns, train=True, get_prenext=False, PRESET=preset, AUG={"SCALE_FACTOR": 0.25, "ROT_FACTOR": 30, "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3})
    cfg = edict({
        "DATASET": {"TRAIN": {"TYPE": "FrameVideo"}, "EVAL": {"TYPE": "FrameVideo"}},
        "DATA_PRESET": {"TYPE": "simple", "SIGMA": 2, "NUM_JOINTS": 17, "IMAGE_SIZE": [256, 192], "HEATMAP_SIZE": [64, 48]},
        "MODEL": dict(SIMPLE_R50), "LOSS": {"TYPE": "MSELoss"}, "AE": {"Z_DIM": 4, "INPUT_DIM": 42, "PRETRAINED": "", "EPOCH": 1, "LR": 1e-3},
        "RETRAIN": {"BATCH_SIZE": 120, "BASE": 1, "OPTIMIZER": "AdamW", "LR": 2.5e-4, "ALPHA": 2, "WEIGHT_DECAY": 0.7, "LR_GAMMA": 0.99},
        "VAL": {"BATCH_SIZE": 256, "W_UNC": 0.01, "UNC_LAMBDA": 0.01, "QUERY_RATIO": [0.05, 0.1, 1.0]}})
    with tempfile.TemporaryDirectory() as wd:
        opt = types.SimpleNamespace(work_dir=wd, uncertainty="THC+WPU", representativeness="None", filter="None", strategy="THC+WPU", video_id="syn",
                                    get_prenext=True, from_scratch=True, continual=True, num_gpu=1, onebyone=False, retrain_thresh=1, THCvsWPU="const")
        torch.manual_seed(0); np.random.seed(0)
        al = ActiveLearning(cfg, opt, eval_dataset=ev, train_dataset=tr)
        n = len(ev)

        def evaluate():
            al.unlabeled_id, al.labeled_id = list(range(n)), []
            al.eval_and_query()
        evaluate()                                          # warm-up: plans, pinned buffers, the data-set fields of the records
        al.flush_records()
        torch.cuda.synchronize()
        single = []
        for _ in range(2):                                  # one call on its own, its record files included
            t0 = time.perf_counter()
            evaluate(); al.flush_records()
            torch.cuda.synchronize(); single.append(time.perf_counter() - t0)
        per_round, traces, gc_passes, gc_t = [], [], [], [0.0]
        import gc

        def on_gc(phase, info):                             # every pass of the cyclic collector that falls into the timed rounds: (round, generation, ms)
            if phase == "start":
                gc_t[0] = time.perf_counter()
            else:
                gc_passes.append((len(per_round), info["generation"], round(1e3 * (time.perf_counter() - gc_t[0]), 2)))
        # Benchmark hygiene, not a product switch: start the timed rounds from a collected heap.  A full (generation-2) pass of CPython's collector over a
        # process that has imported torch costs ~110 ms wherever it lands (r06_bench_b.json: one of eight 71 ms rounds took 179 ms, `collector_passes_over_1ms`
        # showed a 107.7 ms generation-2 pass inside it); WHEN it lands depends on everything this process allocated before — the headline, configs 3 - 5 — not on
        # the rounds.  The passes that still fall into the rounds are reported below; `opt.gc_freeze` stays off (the product default).
        gc.collect()
        evaluate()                                          # (untimed: the pass above left the device idle for ~0.1 s and its clocks down — r06_bench_c.json: 94 ms for the first round after it, 71 after)
        gc.callbacks.append(on_gc)
        t0 = time.perf_counter()
        for _ in range(rounds):                             # back to back: the record files of round r are written inside the device waits of round r + 1
            t1 = time.perf_counter()
            al._trace = []
            evaluate()
            per_round.append(time.perf_counter() - t1)
            traces.append([(lb, round(1e3 * (t - t1), 1)) for lb, t in al._trace])
        al.__dict__.pop("_trace", None)
        al.flush_records()                                  # ... and the last round's inside the timed region
        torch.cuda.synchronize()
        sustained = (time.perf_counter() - t0) / rounds
        gc.callbacks.remove(on_gc)
        slow = max(range(rounds), key=lambda i: per_round[i])
        for name in ("predicted_kpt.json", "predicted_kpt_ann.json", "GT_kpt.json"):
            assert os.path.getsize(os.path.join(wd, name)) > 1000 * n // 4, name
        al.retrain_id = list(range(n)); al.labeled_id = list(range(n)); al.retrain_epoch = 1
        steps = -(-n // cfg.RETRAIN.BATCH_SIZE)
        rt = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            al.retrain_model()
            torch.cuda.synchronize(); rt.append(time.perf_counter() - t0)
    out = {"workload": "ActiveLearning.eval_and_query / retrain_model on 1024 decoded items (uint8 frames -> device crops -> SimpleBaseline-R50 -> THC+WPU scores -> "
                       "record files -> query; fine-tune epoch of 9 x 120 with the auto-encoder refit), wall clock, host work included",
           "items": n, "eval_batch": 256, "eval_and_query_items_per_s": round(n / sustained, 1), "eval_and_query_ms": round(sustained * 1e3, 2),
           "eval_and_query_single_call_items_per_s": round(n / min(single), 1), "eval_and_query_rounds": rounds,
           "eval_and_query_median_round_ms": round(sorted(per_round)[len(per_round) // 2] * 1e3, 2),
           "eval_and_query_p90_round_ms": round(sorted(per_round)[min(len(per_round) - 1, int(0.9 * len(per_round)))] * 1e3, 2),
           "eval_and_query_round_ms": [round(t * 1e3, 2) for t in per_round], "gc_freeze": bool(getattr(opt, "gc_freeze", False)), "gc_collect_before_timed_rounds": True,
           "collector_passes_over_1ms": [g for g in gc_passes if g[2] > 1.0],            # (round, generation, ms)
           "slowest_round": slow, "slowest_round_checkpoints_ms": traces[slow],
           "median_round_checkpoints_ms": traces[sorted(range(rounds), key=lambda i: per_round[i])[rounds // 2]],
           "retrain_model_ms_per_step": round(min(rt[1:]) / steps * 1e3, 2), "retrain_model_steps": steps, "retrain_batch": 120}
    del al, ev, tr
    torch.cuda.empty_cache()
    return out


def extra_configs(dev, world, rank, dist_on):
    """Every rank runs these (the collectives inside need all of them); rank 0 reports."""
    out = {}
    out["cfg3_simplepose_r50_finetune"] = extra_finetune(
        dev, "SimpleBaseline-R50 256x192 fine-tune step: train-mode fwd + masked MSE + bwd + AdamW(3 groups), data-parallel", SIMPLE_R50,
        (256, 192), 120, GFLOP_FWD["simplepose_r50"], (("final_layer", 10), ("preact", 1), ("deconv_layers", 5)), world, dist_on)
    out["cfg4_hrnet_w32_thc_wpu"] = extra_hrnet_shard(dev, world, rank, dist_on)
    out["cfg5_fastpose_r152_384_finetune"] = extra_finetune(
        dev, "FastPose-R152 384x288 fine-tune step: train-mode fwd + masked MSE + bwd + AdamW(4 groups), data-parallel", FAST_R152,
        (384, 288), 32, GFLOP_FWD["fastpose_r152_384"], (("conv_out", 10), ("preact", 1), ("duc1", 5), ("duc2", 5)), world, dist_on, steps=5)
    # the reference-shaped entry points (host work included); single process only: under the N-rank launch the ranks of this script are not an ActiveLearning job
    out["product_entry_points"] = extra_product_entry_points(dev) if (world == 1 and not dist_on) else None
    return out


DUMP_HEATMAP_FRAMES = 128        # heat-maps written by --dump-outputs: 128 of the 1024 frames (27 MB), picked by a fixed seed


def dump_outputs(out_dir, s, hm_buf):
    """The timed path's results of one step (active_learning.scoring.Scores + the heat-maps it scored) as <name>.npy, float32 / float64 only.
    The full heat-map tensor (214 MB) is cut to a seeded sample of whole frames, written with the frame indices it holds."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    frames = np.sort(np.random.default_rng(166).choice(FRAMES, DUMP_HEATMAP_FRAMES, replace=False))
    arrays = {"keypoints": s.keypoints, "argmax": s.argmax.to(torch.float64), "hp": s.hp, "pose_score": s.pose_score, "localpeak": s.localpeak,
              "thc": s.thc, "heatmaps_sample": hm_buf[torch.from_numpy(frames).to(hm_buf.device)], "heatmaps_sample_frames": torch.from_numpy(frames).double()}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------------------------------
# launch
# ---------------------------------------------------------------------------------------------------------------------

def launch_ranks(n: int) -> int:
    """`bench.py --gpus N` run bare: start N fresh rank processes of this script (nothing in this process has touched a GPU:
    importing torch and counting devices do not), relay rank 0's JSON line, fail if any rank fails."""
    backend = os.environ.get("VATL_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and ndev < n:
        print(f"bench.py --gpus {n}: only {ndev} GPU(s) visible (RCCL needs one device per rank)", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=(r == 0)))
    lines = []
    reader = threading.Thread(target=lambda: lines.extend(procs[0].stdout.readlines()), daemon=True)
    reader.start()
    rc = 0
    while any(p.poll() is None for p in procs):
        bad = [p for p in procs if p.poll() not in (None, 0)]
        if bad:                                             # one rank died: the others would wait in a collective forever
            rc = bad[0].returncode or 1
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.2)
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    reader.join(timeout=10)
    for line in lines:
        sys.stdout.write(line)
    sys.stdout.flush()
    if rc == 0 and not any(l.startswith("{") for l in lines):
        rc = 1
    return rc


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the headline: roofline pass + sampled shader clock, headline variants + configs[2..4] (`extra`), CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the headline variants and the configs[2..4] measurements")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's results as DIR/<name>.npy (rank 0)")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


def main():
    a = parse_args()

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: launch one rank per GPU (or run bare and let --gpus start them)")
    dist = world > 1
    if dist:                                            # N ranks share the host: keep torch's CPU pools (model initialisation) from oversubscribing it
        torch.set_num_threads(max(1, granted_cpus()[0] // world))
    ndev = torch.cuda.device_count()
    local = local % max(ndev, 1)                        # (a 1-GPU box can host a 2-rank smoke run: VATL_DIST_BACKEND=gloo)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    backend = os.environ.get("VATL_DIST_BACKEND", "nccl")               # "nccl" is RCCL over xGMI on MI355X
    if dist:
        import torch.distributed as td
        if backend == "nccl":
            td.init_process_group("nccl", device_id=dev)
        else:
            td.init_process_group(backend)

    model = build_model(dev)
    x, bbox, is_prev, is_next = make_video(dev, 166 + rank)
    hm_buf = torch.empty((FRAMES, 17, 64, 48), device=dev)
    gathered = torch.empty((world * FRAMES, 71), device=dev) if dist and backend == "nccl" else None

    def step():
        s = one_step(model, x, bbox, is_prev, is_next, hm_buf)
        if dist:                                        # the only exchange: ~290 B of results per item
            row = torch.cat([s.keypoints.reshape(FRAMES, -1), s.argmax.float(), s.hp[:, None], s.thc[:, None], s.localpeak[:, None]], 1).contiguous()
            if gathered is not None:
                td.all_gather_into_tensor(gathered, row)
            else:                                       # gloo smoke runs: all_gather is host-only there
                row = row.cpu()
                td.all_gather([torch.empty_like(row) for _ in range(world)], row)
        return s

    for _ in range(a.warmup):
        step()
    if dist:
        td.barrier()
    torch.cuda.synchronize()
    clock = ClockSampler(local) if (rank == 0 and a.full) else None
    if clock is not None:
        clock.__enter__()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        last = step()
    torch.cuda.synchronize()
    if dist:
        td.barrier()
    dt = time.perf_counter() - t0
    if clock is not None:
        clock.__exit__()
    if dist:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        dt = float(t.item())
    if a.dump_outputs and rank == 0:                    # before anything else reuses hm_buf
        dump_outputs(a.dump_outputs, last, hm_buf)

    # --full: the measurements that take runs of their own (a plain run goes straight on to the result line)
    roof = conv_roofline(model, x, bbox, is_prev, is_next, hm_buf) if (rank == 0 and a.full) else None
    if roof is not None:
        # the whole step (conv + pool + layout + scorers + launch gaps) against the FLOPs its conv launches execute: the step-level roofline fraction
        roof["e2e_frac"] = round(roof["executed_flops_per_step"] * a.steps / dt / 1e12 / PEAK_FP32_MFMA, 4)
        roof["e2e_algorithmic_frac"] = round(a.steps * FRAMES / dt * GFLOP_PER_CROP * 1e9 / 1e12 / PEAK_FP32_MFMA, 4)
        # `peak` is the SPEC figure (2.4 GHz).  What the silicon sustains under this load is lower (power management): the clock sampled over the
        # timed region gives the peak the matrix pipe could have reached at the clock it actually ran at, and the fractions against THAT — the number
        # that says how much of the remaining distance is kernel and how much is clock.  `frac` itself stays the spec-peak fraction.
        roof.update(clock.summary())
        if roof.get("sclk_mhz_mean"):
            at = PEAK_FP32_MFMA * roof["sclk_mhz_mean"] / NOMINAL_SCLK_MHZ
            roof["nominal_sclk_mhz"] = NOMINAL_SCLK_MHZ
            roof["peak_at_sclk"] = round(at, 2)
            roof["frac_at_sclk"] = round(roof["achieved"] / at, 4)
            roof["e2e_frac_at_sclk"] = round(roof["executed_flops_per_step"] * a.steps / dt / 1e12 / at, 4)
    run_extra = a.full and not a.no_extra
    variants = headline_variants(model, x, bbox, is_prev, is_next, hm_buf) if (rank == 0 and run_extra) else None
    devices = [torch.cuda.get_device_name(dev)]
    if dist:                                            # what actually ran: one entry per rank, gathered (not assumed from --gpus)
        box = [None] * world
        td.all_gather_object(box, {"rank": rank, "device": local, "name": torch.cuda.get_device_name(dev), "backend": td.get_backend()})
        devices = box
    del model, x, hm_buf
    torch.cuda.empty_cache()
    extra = None
    if run_extra:
        if dist:
            td.barrier()
        extra = extra_configs(dev, world, rank, dist)
    if rank == 0:
        line = {
            "metric": "frames/sec pose-infer+uncertainty, 256x192 17-kp", "value": round(a.steps * FRAMES * world / dt, 1),
            "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "SimpleBaseline-R50 256x192 inference + decode + local-peak + THC-L1, 1024-frame synthetic video per GPU",
                       "frames_per_gpu": FRAMES, "batch": BATCH, "tracks": TRACKS, "parallelism": f"frame-sharded x{world}"},
            "world_size_seen": td.get_world_size() if dist else 1, "rank_devices": devices,
        }
        if roof is not None:
            line["roofline"] = roof
        if extra is not None:
            extra["headline_variants"] = variants
            line["extra"] = extra
        if a.full and world == 1 and not a.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline()
        print(json.dumps(line), flush=True)
    if dist:
        td.barrier()                                    # rank 0 was busy with the roofline pass: leave together
        td.destroy_process_group()


if __name__ == "__main__":
    main()
