"""Golden fixtures on disk: every file of tests/golden/ stays under PART_BYTES.

A fixture ``NAME`` is the record ``{key: array}`` that ``tests/golden/make_golden.py`` computes.  ``save`` writes it as
``NAME.npz`` and, when that would exceed PART_BYTES, further parts ``NAME.1.npz``, ``NAME.2.npz`` ...; an array that
does not fit into one part by itself is cut along its first axis into rows stored as ``key#0``, ``key#1`` ...
``load`` reads every part and joins the rows again: the arrays it returns equal the saved ones bit for bit.
"""
from __future__ import annotations

import glob
import io
import os
import re

import numpy as np

PART_BYTES = 1_000_000      # compressed bytes per part (the repository admits no file above 1 MiB)


def _packed_size(a: np.ndarray) -> int:
    b = io.BytesIO()
    np.savez_compressed(b, x=a)
    return b.getbuffer().nbytes


def parts(folder: str, name: str):
    """The files of fixture ``name`` in ``folder``, NAME.npz first."""
    more = [p for p in glob.glob(os.path.join(glob.escape(folder), glob.escape(name) + ".*.npz"))
            if re.fullmatch(re.escape(name) + r"\.\d+\.npz", os.path.basename(p))]
    more.sort(key=lambda p: int(os.path.basename(p)[len(name) + 1:-4]))
    return [os.path.join(folder, name + ".npz")] + more


def save(folder: str, name: str, rec: dict) -> list:
    pieces = []
    for key, a in rec.items():
        a = np.asarray(a)
        if "#" in key:
            raise ValueError(f"fixture key {key!r} contains '#'")
        n = _packed_size(a)
        if n <= PART_BYTES:
            pieces.append((key, a, n))
            continue
        if a.ndim == 0 or a.shape[0] < 2:
            raise ValueError(f"{name}: {key} ({n} bytes packed) cannot be cut along its first axis")
        for r in range(a.shape[0]):
            row = a[r:r + 1]
            m = _packed_size(row)
            if m > PART_BYTES:
                raise ValueError(f"{name}: row {r} of {key} is {m} bytes packed, above {PART_BYTES}")
            pieces.append((f"{key}#{r}", row, m))
    bins = [[{}, 0]]
    for key, a, n in pieces:                 # first fit, in record order
        for b in bins:
            if b[1] + n <= PART_BYTES:
                break
        else:
            b = [{}, 0]
            bins.append(b)
        b[0][key] = a
        b[1] += n
    for old in parts(folder, name):
        if os.path.exists(old):
            os.remove(old)
    out = []
    for i, (d, _) in enumerate(bins):
        path = os.path.join(folder, f"{name}.npz" if i == 0 else f"{name}.{i}.npz")
        np.savez_compressed(path, **d)
        out.append(path)
    return out


def load(folder: str, name: str) -> dict:
    raw = {}
    for path in parts(folder, name):
        with np.load(path) as z:
            for k in z.files:
                if k in raw:
                    raise ValueError(f"{name}: {k} stored twice")
                raw[k] = z[k]
    rec, rows = {}, {}
    for k, a in raw.items():
        if "#" in k:
            key, r = k.split("#")
            rows.setdefault(key, {})[int(r)] = a
        else:
            rec[k] = a
    for key, d in rows.items():
        if key in rec or sorted(d) != list(range(len(d))):
            raise ValueError(f"{name}: rows of {key} are incomplete")
        rec[key] = np.concatenate([d[r] for r in range(len(d))], axis=0)
    return rec
