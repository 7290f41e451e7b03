"""Opt-in flip testing of the evaluation stream on the device.

AlphaPose's validation runs the pose network on a crop and on its mirror image, flips the mirrored heat-maps back with the left / right
joints exchanged (``flip_heatmap(..., shift=True)``, transforms.py:486-518) and lets the decoder average the two
(``hms = (hms + hms_flip) / 2``, :550-552).  ``flip_forward_into`` does that through the entry points the evaluation stream already
uses, in two forwards and two small launches a chunk (csrc/flip.hip): the merged maps have the bits of the reference's own functions
applied to the two forwards.

It stands BESIDE the product path: nothing calls it unless ``cfg.VAL.FLIP_TEST`` (or ``pretrain.py --flip-test``) asks for it.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import vatl_hip as vh

from . import hip_engine, hip_engine_h16


def _entry_points(dtype):
    """(heat-maps only, heat-maps + embedding) of the fp32 engine (``dtype`` None) or of the 16-bit route."""
    if dtype is None:
        return hip_engine.forward_into, hip_engine.forward_with_embedding
    if dtype not in hip_engine_h16.DTYPES:
        raise vh.VatlError(f"flip_forward_into: dtype must be None, torch.float16 or torch.bfloat16, got {dtype}")
    return (lambda m, x, out: hip_engine_h16.forward_h16(m, x, out=out, dtype=dtype),
            lambda m, x, out, emb: hip_engine_h16.forward_with_embedding_h16(m, x, out, emb, dtype=dtype))


def flip_forward_into(m: nn.Module, x: torch.Tensor, out: torch.Tensor, joint_pairs, shift: bool = True, emb: torch.Tensor | None = None,
                      dtype=None) -> torch.Tensor:
    """Flip-tested heat-maps of ``x`` (N,3,H,W fp32 crops) into ``out`` (N,J,H/4,W/4, contiguous fp32):

        out = (forward(x) + flip_heatmap(forward(flip(x)), joint_pairs, shift)) / 2

    ``forward`` is ``hip_engine.forward_into`` (``dtype`` None) or ``hip_engine_h16.forward_h16`` (float16 / bfloat16).  ``emb`` (N, 2048),
    when given, receives the embeddings of the UN-mirrored pass, with the bits ``forward_with_embedding`` / ``_h16`` writes.  The batch
    is cut as ``hip_engine`` cuts it; the mirrored crops and their heat-maps live in one chunk's scratch, reused across chunks.  Everything
    is enqueued on the calling stream, without a host synchronisation.  What the underlying entry points refuse (training mode, CPU
    tensors, a model on another device) is refused by them."""
    fwd, fwd_emb = _entry_points(dtype)
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and isinstance(out, torch.Tensor) and out.dim() == 4 and out.shape[0] == x.shape[0]):
        raise vh.VatlError("flip_forward_into: x must be (N,C,H,W) crops and out (N,J,H/4,W/4) with one row per crop")
    if emb is not None and not (isinstance(emb, torch.Tensor) and emb.dim() == 2 and emb.shape[0] == x.shape[0]):
        raise vh.VatlError("flip_forward_into: emb must be (N, channels of the trunk)")
    vh.flip_src_joints(joint_pairs, out.shape[1])                                         # a bad pair is refused before the first forward
    x_flip = hm_flip = None
    for a, b in hip_engine._chunks(x.shape[0], x.shape[2:]):
        xc, oc = x[a:b], out[a:b]
        if emb is None:
            fwd(m, xc, oc)
        else:
            fwd_emb(m, xc, oc, emb[a:b])
        xc = xc.detach().float().contiguous()                                             # what the entry point above has run on
        if x_flip is None:                                                                # the first chunk is the largest
            x_flip, hm_flip = torch.empty_like(xc), torch.empty_like(oc)
        n = b - a
        vh.flip_nchw(xc, out=x_flip[:n])
        fwd(m, x_flip[:n], hm_flip[:n])
        vh.flip_merge(oc, hm_flip[:n], joint_pairs, shift)
    return out
