#!/usr/bin/env python3
"""Generate tests/golden/flip_test.npz by running the REFERENCE's own flip-test helpers on the cases of tests/flip_cases.py (CPU only).

Usage:  python tools/make_flip_golden.py --ref <reference checkout> [--out tests/golden/flip_test.npz]

The reference's ``alphapose/utils/transforms.py`` is imported from ``--ref`` with the import shims of tools/make_golden.py.  Nothing from
the reference is copied: the fixture holds the pair tables, the SHA-256 of the seeded inputs (tests/flip_cases.py regenerates them) and,
per case, what the reference made of them:

    <case>.flip          flip(hm)                                                  transforms.py:479-483
    <case>.fh0           flip_heatmap(hm_flip, pairs, shift=False)                 :486-518
    <case>.fh1           ... with the shift of :513-517, see below
    <case>.m0 / .m1      (hm + fh) / 2, the line of heatmap_to_coord_simple        :552
    order.<table>        flip_heatmap of planes that hold their joint number: the joint each output joint comes from
    decode.coords / .maxvals   heatmap_to_coord_simple(hm[n], box[n], hms_flip=fh1[n]) of the DECODE_CASE planes

The shift.  The reference writes it as ``out[:, :, :, 1:] = out[:, :, :, 0:-1]``: source and destination are views of ONE tensor, one
pixel apart.  torch refuses such a copy where it can tell (contiguous views); for these strided 4-D views it cannot and runs its copy
loop over memory that changes under it, so for W > 2 the outcome depends on how that loop happens to be vectorised (on the CPU build this
script was written on, W = 5 rows come out as pixel 0 repeated and a third of the pixels of W = 48 rows differ), not on the statement.  The fixture therefore takes
the statement at its value: the right-hand side is read before anything is written, as NumPy evaluates the same line and as the
restatement in this repository does (``.clone()``) — applied here to the reference's own ``shift=False`` output, with two DISTINCT tensors.
For W <= 2, where the aliased copy moves a single pixel and is defined, the reference's own ``shift=True`` call is asserted to agree.

Arrays of more than DIGEST_ABOVE words are stored as their SHA-256.  Before anything is written, the numpy model of tests/flip_cases.py
(which states csrc/flip.hip's formula) must reproduce every reference output bit for bit.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import make_golden  # noqa: E402  (the shims)
from tests import flip_cases as FC  # noqa: E402


def put(store, key, a):
    a = np.ascontiguousarray(a)
    store[key] = a if a.size <= FC.DIGEST_ABOVE else np.array(FC.digest(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=FC.GOLDEN)
    a = ap.parse_args()
    make_golden.install_shims()
    sys.path.insert(0, a.ref)
    from alphapose.utils import transforms as T                   # the reference's
    assert os.path.abspath(T.__file__).startswith(os.path.abspath(a.ref)), T.__file__

    store = {}
    for table, pairs in FC.TABLES.items():
        store[f"pairs.{table}"] = np.asarray(pairs, np.int64).reshape(-1, 2)
        j = 17 if pairs else 15
        planes = torch.arange(j, dtype=torch.float32).reshape(1, j, 1, 1).repeat(1, 1, 2, 3)
        order = T.flip_heatmap(planes, [list(p) for p in pairs], shift=False)[0, :, 0, 0].numpy().astype(np.int64)
        assert list(order) == FC.src_joints(pairs, j), (table, order)
        store[f"order.{table}"] = order
    for name, (n, j, h, w, table, seed) in FC.CASES.items():
        pairs = [list(p) for p in FC.TABLES[table]]
        hm, fl = FC.inputs(name)
        store[f"{name}.hm_sha"], store[f"{name}.fl_sha"] = np.array(FC.digest(hm)), np.array(FC.digest(fl))
        flipped = T.flip(torch.from_numpy(hm)).numpy()
        assert np.array_equal(flipped.view(np.int32), hm[..., ::-1].view(np.int32)), name
        put(store, f"{name}.flip", flipped)
        for s in (0, 1):
            fh = T.flip_heatmap(torch.from_numpy(fl.copy()), pairs, shift=False)
            if s:                                                  # :517 at its value (see the module docstring)
                unshifted = fh.clone()
                fh[:, :, :, 1:] = unshifted[:, :, :, 0:-1]
                if w <= 2:
                    assert FC.same_bits(T.flip_heatmap(torch.from_numpy(fl.copy()), pairs, shift=True).numpy(), fh.numpy()), name
            m = ((torch.from_numpy(hm) + fh) / 2).numpy()          # heatmap_to_coord_simple's `hms = (hms + hms_flip) / 2`
            fh = fh.numpy()
            assert FC.same_bits(FC.flip_heatmap_model(fl, pairs, s), fh), (name, s)
            assert FC.same_bits(FC.merge_model(hm, fl, pairs, s), m), (name, s)
            put(store, f"{name}.fh{s}", fh)
            put(store, f"{name}.m{s}", m)
        if name == FC.DECODE_CASE:
            bb = FC.boxes(n)
            coords, maxvals = [], []
            for i in range(n):
                c, v = T.heatmap_to_coord_simple(torch.from_numpy(hm[i]), bb[i], hms_flip=torch.from_numpy(fh[i]))   # fh: shift=True
                coords.append(c)
                maxvals.append(v)
            store["decode.coords"], store["decode.maxvals"] = np.asarray(coords, np.float32), np.asarray(maxvals, np.float32)
    np.savez_compressed(a.out, **store)
    print(f"{a.out}: {len(store)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
