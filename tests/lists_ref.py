"""Definitions of the index-list primitives (csrc/ddp_lists.hip, csrc/ddp_views.hip) in numpy int64, written from the comments of
include/ddp_hip.h - one function per entry point.  Every function returns, per output array, an `Out`: the positions the kernel
may write and the values the definition puts there (`val is None`: workspace, any value).  Positions outside `idx` must keep
whatever they held before the call.  Nothing here calls the library or graph.py."""
from typing import NamedTuple, Optional

import numpy as np


class Out(NamedTuple):
    idx: np.ndarray             # int64, distinct positions of the (flattened) output array
    val: Optional[np.ndarray]   # int64 values expected at idx, or None for workspace


def _a(x):
    return None if x is None else np.asarray(x).astype(np.int64)


def _ar(n):
    return np.arange(n, dtype=np.int64)


def count(cap, n_dev=None):
    """The actual item count of a job: the capacity, or the device-side count clamped to [0, capacity]."""
    return int(cap) if n_dev is None else min(max(int(n_dev), 0), int(cap))


def scan(n, n_dev=None, flag=None, val=None, rowptr=None, base=0):
    """ddp_scan_jobs, one job.  Keys: excl [0, n], excl2 [0, n), total, and - for 0 / 1 values - list."""
    n = count(n, n_dev)
    flag, val, rowptr = _a(flag), _a(val), _a(rowptr)
    v = np.ones(n, dtype=np.int64)
    if val is not None:
        v = val[:n].copy()
    elif rowptr is not None:
        v = rowptr[1:n + 1] - rowptr[:n]
    if flag is not None:
        v = np.where(flag[:n] != 0, v, 0)
    e = base + np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(v)])
    out = {"excl": Out(_ar(n + 1), e), "excl2": Out(_ar(n), e[:n]), "total": Out(_ar(1), e[n:])}
    if val is None and rowptr is None:
        k = np.nonzero(v)[0].astype(np.int64)
        out["list"] = Out(e[k], k)
    return out


def mark(n, n_dev=None, idx=None):
    """ddp_mark_jobs, one job: mask[idx[i]] = 1 for i < n (idx None: mask[i] = 1)."""
    n = count(n, n_dev)
    t = _ar(n) if idx is None else np.unique(_a(idx)[:n])
    return {"mask": Out(t, np.ones(t.shape[0], dtype=np.int64))}


def rowcopy(n_rows, keep, old_rowptr, new_rowptr, ins):
    """ddp_rowcopy_jobs, one job: a kept row's entries move, in order, from old_rowptr[r] .. to new_rowptr[r] ..."""
    keep, old, new = _a(keep), _a(old_rowptr), _a(new_rowptr)
    rows = np.nonzero(keep[:n_rows])[0]
    lens = old[rows + 1] - old[rows]
    rep = np.repeat(rows, lens)
    a = _ar(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    src, dst = old[rep] + a, new[rep] + a
    return {"outs": [Out(dst, _a(x)[src]) for x in ins]}


def select(n, n_dev=None, mask_a=None, idx_a=None, mask_b=None, idx_b=None, pays=(), pay_add=None):
    """ddp_select_jobs, one job: the items with mask_a[idx_a ? idx_a[i] : i] | mask_b[idx_b ? idx_b[i] : i], in ascending i."""
    n = count(n, n_dev)
    i = _ar(n)
    f = np.zeros(n, dtype=bool)
    for m, ix in ((mask_a, idx_a), (mask_b, idx_b)):
        if m is not None:
            f |= _a(m)[i if ix is None else _a(ix)[:n]] != 0
    k = np.nonzero(f)[0].astype(np.int64)
    j = _ar(k.shape[0])
    add = [0] * len(pays) if pay_add is None else pay_add
    return {"out_idx": Out(j, k), "outs": [Out(j, _a(p)[k] + add[q]) for q, p in enumerate(pays)],
            "total": Out(_ar(1), np.array([k.shape[0]], dtype=np.int64))}


def gather_rows(x, idx, n, n_dev, ncols, ldo):
    """ddp_gather_rows: out[i, :ncols] = x[idx[i], :ncols] for i < n; x [rows, ldx] as 32-bit patterns, out flattened with ldo."""
    n = count(n, n_dev)
    x, idx = _a(x), _a(idx)
    pos = (_ar(n)[:, None] * ldo + _ar(ncols)[None, :]).reshape(-1)
    return {"out": Out(pos, x[idx[:n], :ncols].reshape(-1))}


def clean_pair_maps(touched, recv, src, n_edges, e0, n_graphs, n0, rowptr=None):
    """ddp_clean_pair_maps: rowmap[p] = p if an end of edge p is touched, else E + (the same edge's position in sample 0's list:
    p % e0, or with rowptr the receiver's row in sample 0 at the same offset); rows_v[a0] = g * n0 + a0, g the first sample in
    which atom a0 is untouched (0 if there is none)."""
    touched, recv, src, rowptr = _a(touched), _a(recv), _a(src), _a(rowptr)
    p = _ar(n_edges)
    ref = p % e0 if rowptr is None else rowptr[recv % n0] + (p - rowptr[recv])
    dirty = (touched[recv] != 0) | (touched[src] != 0)
    clean = touched[:n_graphs * n0].reshape(n_graphs, n0) == 0
    g = np.where(clean.any(0), clean.argmax(0), 0)
    return {"rowmap": Out(p, np.where(dirty, p, n_edges + ref)), "rows_v": Out(_ar(n0), g * n0 + _ar(n0))}


def flex_mark(a, b, n_edges, e0, n_a, n_b, pos=None, flag=None, a_too=False, ref_list=False):
    """ddp_flex_mark.  pos: [nodes, 3] as 32-bit patterns ("off" = differs BITWISE from sample 0's), or flag [nodes]."""
    a, b, flag = _a(a)[:n_edges], _a(b)[:n_edges], _a(flag)
    pos = None if pos is None else np.asarray(pos).astype(np.int64)
    e = _ar(n_edges)
    s = e // e0

    def off(x):                 # node x of the b kind, in the sample s of the edge
        if flag is not None:
            return flag[x] != 0
        return (pos[x] != pos[x - s * n_b]).any(1)

    live = s > 0
    m = off(b)
    if a_too:
        m = m | off(a)
    marks = [_ar(n_a), a[m & live]]
    if ref_list:
        l = e - s * e0
        m2 = off(b[l] + s * n_b) & live
        marks.append((a[l] + s * n_a)[m2])
    t = np.unique(np.concatenate(marks))
    return {"mark": Out(t, np.ones(t.shape[0], dtype=np.int64))}


def fallback_rowmap(mark, recv, old_rowptr, new_rowptr, n_edges, n_recv):
    """ddp_fallback_rowmap: rowmap[p] = new_rowptr[t] + (p - old_rowptr[r]), r = recv[p], t = mark[r] ? r : r % n_recv."""
    mark, r, old, new = _a(mark), _a(recv)[:n_edges], _a(old_rowptr), _a(new_rowptr)
    p = _ar(n_edges)
    t = np.where(mark[r] != 0, r, r % n_recv)
    return {"rowmap": Out(p, new[t] + (p - old[r]))}


def group_by_key(key, n_items, n_dev, n_keys, pays=(), key_map=None, perm=True):
    """ddp_group_by_key_jobs, one job: the stable sort of the first n items by key plus the row pointers.  perm False: rowptr only."""
    n = count(n_items, n_dev)
    k = _a(key)[:n] if n else np.zeros(0, dtype=np.int64)
    rp = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.bincount(k, minlength=n_keys))])
    out = {"rowptr": Out(_ar(n_keys + 1), rp), "scratch": Out(_ar(n_keys + (n if perm else 0)), None)}
    if perm:
        order = np.argsort(k, kind="stable").astype(np.int64)
        ok = k if key_map is None else _a(key_map)[k]
        out.update(perm=Out(_ar(n), order), out_key=Out(_ar(n), ok[order]), outs=[Out(_ar(n), _a(p)[order]) for p in pays])
    return out
