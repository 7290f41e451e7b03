"""Opt-in replayable fine-tune step (``cfg.RETRAIN.GRAPH``): forward + masked MSE + backward into the gradient arena as ONE captured
HIP graph per (trainer, input shape, loss scale), for the regime the active-learning loop really runs — a few hundred epochs of one
small batch each, every epoch the same shape, where an eager step is ~500 Python wrapper calls and the device waits for the host.

    step = graphed_step_for(model, precision="fp32" | "bf16")
    out, loss = step(x, labels, masks, scale=1.0)

A call equals, bit for bit, what ``ActiveLearning.retrain_model`` runs for a single chunk:

    out = trainer.forward(x); loss, dout = vh.masked_mse_fwd_bwd(out, labels, masks); [dout.mul_(scale)]
    arena.begin(); trainer.backward(dout, arena=arena, overlap=True); arena.finish()

``arena.attach()`` and ``optimizer.step()`` stay with the caller, outside the graph: step count and learning rates are launch arguments.

Life cycle of a (shape, dtype, scale): the first call is a real eager step (it seals the pack plan, packs the lazily packed filters,
fills every cache a wrapper keeps per shape and warms the allocator, so nothing is packed or uploaded for the first time inside a capture);
the second copies the inputs into static buffers, captures the sequence (a capture executes nothing) and replays it; every later call
is copy-in + replay.  ``step.path`` says what the last call did — "eager:warm", "captured", "replayed" or "eager:<reason>" — and
``step.stats`` counts the outcomes.  ``out`` of a captured / replayed call is the graph's static heat-map buffer: valid until the next
call on that shape.  ``loss`` is always a fresh 0-dim tensor.

A graph holds raw pointers and the routes the trainer took while it was captured, so it lives only as long as ``dependency_key``
stays what it was: see there.  At most ``MAX_GRAPHS`` shapes are kept per step object, the least recently used goes first (a retrain
epoch has one full-batch shape and at most one ragged tail).  A capture that raises leaves that shape eager for the life of the step
object — one attempt, no retry; an exception from a replay propagates.

Nothing imports this module unless asked; the default route and every bit it produces are untouched.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

import vatl_hip as vh

from . import hip_train

# Capture with the weight gradients forked onto the trainers' side stream, as the eager step runs them (True), or as a linear
# single-stream graph (False).  Same bits either way (tests/test_gpu_train_fullsize.py pins the single-stream order to the forked
# one).  Measured at B = 24 (profiles/train_graph_notes.md): the linear graph is the faster replay for three of the four
# configurations, HRNet-W32 — the one "auto" serves — among them (30.4 against 32.4 ms).
SIDE_STREAM_IN_GRAPH = False
# cfg.RETRAIN.GRAPH "auto": graphed steps for chunks of at most this many crops, for the networks whose replay beat the parent
# commit's eager step at B = 8 and B = 24 (profiles/train_graph_notes.md: HRNet-W32 only; the SimplePose / FastPose steps are not
# bound by launch issue even at B = 8 and a replay costs them 1.1 - 1.6 ms)
AUTO_MAX_CROPS = 24
AUTO_NETWORKS = ("PoseHighResolutionNet",)


def auto_max_crops(model, precision: str) -> int:
    """The largest chunk ``RETRAIN.GRAPH: auto`` sends through a graph for this network and precision (0: none)."""
    return AUTO_MAX_CROPS if precision == "fp32" and type(model).__name__ in AUTO_NETWORKS else 0
MAX_GRAPHS = 4
_MAX_WARM = 3                                      # eager steps a shape may take before its pack plan must be ready


def route_constants(precision: str):
    """The module constants a trainer reads while it runs, in a fixed order: a captured graph froze the routes they chose."""
    vals = [hip_train._FUSE_BN_BWD, hip_train._WINOGRAD, hip_train._WINOGRAD_F4, hip_train._WINOGRAD_WGRAD_MIN_C, hip_train._FUSE_BN_MIN_C,
            hip_train._USE_PACK_PLAN, hip_train._side.enabled, SIDE_STREAM_IN_GRAPH]
    if precision == "bf16":
        from . import hip_train_h16
        vals.append(hip_train_h16._USE_PACK_PLAN)
    else:
        vals.append(None)
    return tuple(vals)


def dependency_key(ptrs, trainable, training, device, shape, dtype, constants):
    """What a captured step depends on, as one hashable value (a pure function of its arguments; tests/test_train_graph_cpu.py):
    ``ptrs`` — data_ptr() of every parameter and buffer (the captured pack-plan launch and every BatchNorm kernel read the tensors' own
    storage: an in-place load_state_dict keeps them, ``p.data = ...`` does not); ``trainable`` — which parameters have requires_grad
    (the arena's layout); the module's train flag; the device; the input's shape and dtype; the route constants (``route_constants``)."""
    return (tuple(int(p) for p in ptrs), tuple(bool(t) for t in trainable), bool(training), str(device), tuple(int(s) for s in shape), str(dtype),
            tuple(constants))


class _Slot:
    """One (shape, dtype, scale): its place in the life cycle and, once captured, the graph with its static buffers."""

    def __init__(self):
        self.warm = 0
        self.graph = None
        self.x = self.labels = self.masks = self.out = self.loss = None
        self.bumps = ()                            # (tensor, times) whose version counters an eager step bumps on the host


class GraphedStep:
    def __init__(self, model, precision="fp32"):
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        self.model, self.precision = model, precision
        if precision == "bf16":
            from . import hip_train_h16
            self.trainer = hip_train_h16.trainer_for_h16(model)            # refuses what it refuses, by name
        else:
            self.trainer = hip_train.trainer_for(model)
        self._has_dcn = any(getattr(mod, "with_dcn", False) for mod in model.modules())
        self.path = None
        self.stats = {"eager": 0, "captured": 0, "replayed": 0}
        self.reasons = []                          # distinct "eager:<reason>" texts, in order of first appearance
        self._slots = OrderedDict()                # (shape, dtype, scale) -> _Slot, least recently used first
        self._failed = {}                          # (shapes, dtype, scale) -> reason: eager for the life of this object
        self._model_part = None                    # the part of dependency_key that does not belong to one input shape
        self._stream = None                        # where warm steps and captures run

    # ------------------------------------------------------------------ the sequence
    def _sequence(self, x, labels, masks, scale):
        arena = hip_train.arena_for(self.model)
        with torch.no_grad():
            out = self.trainer.forward(x)
            loss, dout = vh.masked_mse_fwd_bwd(out, labels, masks)
            if scale != 1.0:
                dout.mul_(scale)
            arena.begin()
            self.trainer.backward(dout, arena=arena, overlap=True)
            arena.finish()
        return out, loss

    def _eager(self, x, labels, masks, scale, why):
        self.path = "eager:" + why
        self.stats["eager"] += 1
        if why != "warm" and self.path not in self.reasons:
            self.reasons.append(self.path)
        out, loss = self._sequence(x, labels, masks, scale)
        return out, loss.reshape(())

    def _warm(self, x, labels, masks, scale):
        """An eager step on the stream the capture will use, so that whatever a trainer remembers about streams (the bf16 pack plan
        waits, at its next begin(), for the streams its kept buffers were last read on) needs no wait across the capture's boundary."""
        cur = torch.cuda.current_stream(x.device)
        st = self._capture_stream(x.device)
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            out, loss = self._eager(x, labels, masks, scale, "warm")
        cur.wait_stream(st)
        out.record_stream(cur); loss.record_stream(cur)
        return out, loss

    def _capture_stream(self, device):
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=device)
        return self._stream

    # ------------------------------------------------------------------ what keeps a step eager
    def _refusal(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return "world size > 1: the arena's all-reduce is not captured"
        if hip_train._relu_tap is not None:
            return "hip_train._relu_tap records the ReLU masks"
        if vh.STREAMK_IN_TRAINING:
            return "vatl_hip.STREAMK_IN_TRAINING is set"
        if self._has_dcn:
            return "deformable bottlenecks (DCN): their backward pass is not covered"
        return None

    def _dependency(self, x):
        m = self.model
        params = list(m.parameters())
        ptrs = [p.data_ptr() for p in params] + [b.data_ptr() for b in m.buffers()]
        return dependency_key(ptrs, [p.requires_grad for p in params], m.training, x.device, x.shape, x.dtype, route_constants(self.precision))

    def _plan_ready(self):
        """Whether the trainer's pack plan would replay (one launch, kept buffers) in the next forward pass: only then is a capture free
        of first-time packs and of the table upload."""
        if self.precision == "bf16":
            from . import hip_train_h16
            on = hip_train_h16._USE_PACK_PLAN
        else:
            on = hip_train._USE_PACK_PLAN
        if not on:
            return True                            # per-tensor packs: plain launches into fresh buffers
        plan = self.trainer.__dict__.get("_pack_plan")
        return plan is not None and plan.ready and not plan.stale

    # ------------------------------------------------------------------ the call
    def __call__(self, x, labels, masks, scale=1.0):
        scale = float(scale)
        why = self._refusal()
        if why is not None:
            return self._eager(x, labels, masks, scale, why)
        shape_key = (tuple(x.shape), x.dtype, tuple(labels.shape), tuple(masks.shape), scale)
        if shape_key in self._failed:
            return self._eager(x, labels, masks, scale, self._failed[shape_key])
        dep = self._dependency(x)
        model_part = dep[:4] + dep[6:]
        if model_part != self._model_part:
            # storage, trainable set, train flag, device or a route constant changed: every graph of this step object is stale
            self._slots.clear()
            self._model_part = model_part
        key = (dep,) + shape_key[2:]
        slot = self._slots.get(key)
        if slot is None:
            slot = self._slots[key] = _Slot()
            while len(self._slots) > MAX_GRAPHS:
                self._slots.popitem(last=False)
        self._slots.move_to_end(key)
        if slot.graph is not None:
            return self._replay(slot, x, labels, masks, bump=True)
        if slot.warm == 0 or (not self._plan_ready() and slot.warm < _MAX_WARM):
            slot.warm += 1
            return self._warm(x, labels, masks, scale)
        if not self._plan_ready():
            del self._slots[key]
            self._failed[shape_key] = f"the pack plan was not ready after {_MAX_WARM} eager steps"
            return self._eager(x, labels, masks, scale, self._failed[shape_key])
        try:
            self._capture(slot, x, labels, masks, scale)
        except Exception as e:                                                       # noqa: BLE001 - one attempt; the text goes into ``path``
            self._after_failed_capture()
            del self._slots[key]
            self._failed[shape_key] = "capture failed: " + f"{type(e).__name__}: {e}"[:300]
            return self._eager(x, labels, masks, scale, self._failed[shape_key])
        self.stats["captured"] += 1
        out = self._replay(slot, x, labels, masks, bump=False, copy=False)               # the capture did this step's host-side bumps
        self.path = "captured"
        return out

    def _capture(self, slot, x, labels, masks, scale):
        stream = self._capture_stream(x.device)
        slot.x, slot.labels, slot.masks = (torch.empty_like(t, memory_format=torch.contiguous_format) for t in (x, labels, masks))
        slot.x.copy_(x); slot.labels.copy_(labels); slot.masks.copy_(masks)
        versions = [(b, b._version) for b in self.model.buffers()]
        graph = torch.cuda.CUDAGraph()
        side = hip_train._side
        keep = side.enabled
        if not SIDE_STREAM_IN_GRAPH:
            side.enabled = False
        try:
            with torch.cuda.graph(graph, stream=stream):
                out, loss = self._sequence(slot.x, slot.labels, slot.masks, scale)
        finally:
            side.enabled = keep
        slot.out, slot.loss, slot.graph = out, loss, graph
        # host-side work of an eager step that a replay repeats by hand: the version counters of the BatchNorm statistics written
        # through raw pointers (hip_train._flush_batch_counters) and of the counters the captured _foreach_add_ bumps
        slot.bumps = tuple((b, b._version - v) for b, v in versions if b._version != v)

    def _after_failed_capture(self):
        """Host-side state a pass that stopped half-way leaves behind: deferred BatchNorm counters (the next flush would count them
        twice) and a side stream marked as in use."""
        hip_train._pending_counters.clear()
        hip_train._pending_stats.clear()
        hip_train._side.used = False

    def _replay(self, slot, x, labels, masks, bump, copy=True):
        if copy:
            slot.x.copy_(x); slot.labels.copy_(labels); slot.masks.copy_(masks)
        slot.graph.replay()
        if bump:
            inc = torch.autograd.graph.increment_version
            for t, n in slot.bumps:
                for _ in range(n):
                    inc(t)
        self.path = "replayed"
        if bump:
            self.stats["replayed"] += 1
        return slot.out, slot.loss.clone().reshape(())


def graphed_step_for(model, precision="fp32") -> GraphedStep:
    """The (cached) graphed step of a pose network, like ``hip_train.trainer_for`` / ``arena_for``."""
    name = "_vatl_graphed_step_" + precision
    step = model.__dict__.get(name)
    if step is None:
        step = model.__dict__[name] = GraphedStep(model, precision)
    return step
