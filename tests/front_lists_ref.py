"""Definition of the step's pose-dependent edge lists (include/ddp_hip.h: ddp_front_lists) in numpy, composed as the chain it
replaces: dense radius searches -> prefix sums -> stable groupings (tests/lists_ref.py), plus the cases the tests run.  Nothing
here calls the library.  Distances are float32 with separately rounded operations, (dx^2 + dy^2) + dz^2, compared strictly."""
from types import SimpleNamespace

import numpy as np

import lists_ref as R
from lists_ref import Out

f32 = np.float32


def _sq(y, x):
    """float32 squared distances [ny, nx], rounded like csrc/ddp_radius_math.h."""
    d = y[:, None, :].astype(f32) - x[None, :, :].astype(f32)
    s = d * d
    return (s[..., 0] + s[..., 1]) + s[..., 2]


def dense_radius(x, x_ptr, y, y_ptr, r, cap, drop_self=False, div=None):
    """radius(x, y, r) per graph: for every query y (ascending) the points x of its graph with d2 < r2 in ascending index, the first
    `cap` of them, the self pair dropped afterwards.  div [graphs]: both sides divided by div[g] first.  Returns (query, point, counts)."""
    r2 = f32(r) * f32(r)
    qs, xs, counts = [], [], np.zeros(y.shape[0], dtype=np.int64)
    for g in range(len(x_ptr) - 1):
        xa, ya = x[x_ptr[g]:x_ptr[g + 1]].astype(f32), y[y_ptr[g]:y_ptr[g + 1]].astype(f32)
        if div is not None:
            xa, ya = xa / f32(div[g]), ya / f32(div[g])
        m = _sq(ya, xa) < r2
        for qi in range(ya.shape[0]):
            j = np.nonzero(m[qi])[0][:cap] + x_ptr[g]
            q = y_ptr[g] + qi
            if drop_self:
                j = j[j != q]
            counts[q] = j.shape[0]
            qs.append(np.full(j.shape[0], q, dtype=np.int64))
            xs.append(j.astype(np.int64))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, dtype=np.int64)        # noqa: E731
    return cat(qs), cat(xs), counts


def naive_radius(x, x_ptr, y, y_ptr, r, cap, drop_self=False, div=None):
    """The same by plain loops over pairs."""
    r2 = f32(r) * f32(r)
    qs, xs = [], []
    for g in range(len(x_ptr) - 1):
        for q in range(y_ptr[g], y_ptr[g + 1]):
            seen = 0
            for j in range(x_ptr[g], x_ptr[g + 1]):
                a, b = y[q].astype(f32), x[j].astype(f32)
                if div is not None:
                    a, b = a / f32(div[g]), b / f32(div[g])
                dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
                if (dx * dx + dy * dy) + dz * dz < r2:
                    seen += 1
                    if seen <= cap and not (drop_self and j == q):
                        qs.append(q)
                        xs.append(j)
    return np.array(qs, dtype=np.int64), np.array(xs, dtype=np.int64)


def naive_group(key, n, n_keys):
    """Stable grouping of the first n items by plain loops: (rowptr, perm)."""
    perm = [i for k in range(n_keys) for i in range(n) if key[i] == k]
    rp = [sum(1 for i in range(n) if key[i] < k) for k in range(n_keys + 1)]
    return np.array(rp, dtype=np.int64), np.array(perm, dtype=np.int64)


def _list(q, x, base, cap, first, second, pre=None):
    """A search's pairs behind `base` existing entries, never at or behind the capacity: Outs of the two arrays + full arrays."""
    n = min(base + q.shape[0], cap)
    idx = np.arange(base, max(n, base), dtype=np.int64)
    full = {}
    for name, v, p in ((first, q, None if pre is None else pre[0]), (second, x, None if pre is None else pre[1])):
        a = np.zeros(max(n, base), dtype=np.int64)
        if base:
            a[:base] = p
        a[base:n] = v[:n - base]
        full[name] = a
    return {first: Out(idx, full[first][base:]), second: Out(idx, full[second][base:])}, full, base + q.shape[0]


def _view(name, key, n, n_keys, pays, o1=False, rowptr=True):
    g = R.group_by_key(key, n, None, n_keys, pays=pays)
    out = {f"{name}.perm": g["perm"], f"{name}.key": g["out_key"], f"{name}.o0": g["outs"][0]}
    if rowptr:
        out[f"{name}.rp"] = g["rowptr"]
    if o1:
        out[f"{name}.o1"] = g["outs"][1]
    return out, g


def front_lists_def(c):
    """All outputs of ddp_front_lists for a case (see `case`): name -> Out."""
    B = c.B
    out = {}
    q, x, _ = dense_radius(c.lpos, c.ptr_l, c.lpos, c.ptr_l, c.r_lig, c.ll_nb, drop_self=True)
    o, ll, tot_ll = _list(q, x, c.Eb, c.cap_ll, "ll1", "ll0", pre=(c.bond1, c.bond0))
    out.update(o)
    q, x, _ = dense_radius(c.rpos, c.ptr_r, c.lpos, c.ptr_l, c.r_cross, 10000, div=c.cut)
    o, lr, tot_lr = _list(q, x, 0, c.cap_lr, "lr0", "lr1")
    out.update(o)
    q, x, _ = dense_radius(c.apos, c.ptr_a, c.lpos, c.ptr_l, c.r_lig, 10000)
    o, la, tot_la = _list(q, x, 0, c.cap_la, "la0", "la1")
    out.update(o)
    out["overflow"] = Out(np.arange(1), np.array([1 if tot_la > c.cap_la else 0]))
    _, _, touched = dense_radius(c.lpos, c.ptr_l, c.apos, c.ptr_a, c.r_lig, 10000)
    out["touched"] = Out(np.arange(c.Na), touched)
    near = R.scan(c.Na, flag=touched)
    out["near_rows"], out["cnt.near"] = near["list"], near["total"]
    out["cnt.ll"], out["cnt.lr"], out["cnt.la"] = (Out(np.arange(1), np.array([t])) for t in (tot_ll, tot_lr, tot_la))
    n_ll, n_lr, n_la = (R.count(cap, t) for cap, t in ((c.cap_ll, tot_ll), (c.cap_lr, tot_lr), (c.cap_la, tot_la)))
    if c.T > 0:
        q, x, _ = dense_radius(c.lpos, c.ptr_l, c.tpos, c.ptr_t, c.r_lig, c.tor_nb)
        o, tr, tot_t = _list(q, x, 0, c.cap_tor, "tor_q", "tor_x")
        out.update(o)
        out["cnt.tor"] = Out(np.arange(1), np.array([tot_t]))
        out["rp_tor"] = R.group_by_key(tr["tor_q"], R.count(c.cap_tor, tot_t), None, c.T, perm=False)["rowptr"]
    # first grouping call
    o, c_ll = _view("c_ll", ll["ll0"], n_ll, c.Nl, [ll["ll1"]])
    out.update(o)
    out["rp_lr"] = R.group_by_key(lr["lr0"], n_lr, None, c.Nl, perm=False)["rowptr"]
    out["rp_la"] = R.group_by_key(la["la0"], n_la, None, c.Nl, perm=False)["rowptr"]
    o, c_la = _view("c_la", la["la1"], n_la, c.Na, [la["la0"]])
    out.update(o)
    o, c_lr = _view("c_lr", lr["lr1"], n_lr, c.Nr, [lr["lr0"]])
    out.update(o)
    # second grouping call: each view grouped by its payload (the source node) with the payloads (key, perm)
    for name, v, n in (("so_ll", c_ll, n_ll), ("so_la", c_la, n_la), ("so_lr", c_lr, n_lr)):
        o, _ = _view(name, v["outs"][0].val, n, c.Nl, [v["out_key"].val, v["perm"].val], o1=True)
        out.update(o)
    assert B == len(c.ptr_l) - 1
    return out


def sizes(c):
    """name -> length of every output array of a case."""
    s = {"ll0": c.cap_ll, "ll1": c.cap_ll, "lr0": c.cap_lr, "lr1": c.cap_lr, "la0": c.cap_la, "la1": c.cap_la, "overflow": 1,
         "touched": c.Na, "near_rows": c.Na, "cnt.ll": 1, "cnt.lr": 1, "cnt.la": 1, "cnt.near": 1, "rp_lr": c.Nl + 1, "rp_la": c.Nl + 1}
    if c.T > 0:
        s.update({"tor_q": c.cap_tor, "tor_x": c.cap_tor, "cnt.tor": 1, "rp_tor": c.T + 1})
    for name, nk, cap in (("c_ll", c.Nl, c.cap_ll), ("c_la", c.Na, c.cap_la), ("c_lr", c.Nr, c.cap_lr), ("so_ll", c.Nl, c.cap_ll),
                          ("so_la", c.Nl, c.cap_la), ("so_lr", c.Nl, c.cap_lr)):
        s.update({f"{name}.rp": nk + 1, f"{name}.perm": cap, f"{name}.key": cap, f"{name}.o0": cap})
        if name.startswith("so"):
            s[f"{name}.o1"] = cap
    return {k: max(v, 1) for k, v in s.items()}


def case(seed, nl, nr, na, nt=None, far=(), cut=None, bonds=True, la_per_atom=None, r_lig=5.0, ll_nb=33, tor_nb=32, ll_short=0):
    """A batch with per-sample sizes nl / nr / na / nt.  Ligand atoms lie in a cube whose diagonal is below r_lig (every pair of a
    sample matches: the cap of ll_nb binds from ll_nb + 1 atoms on), receptor nodes and atoms in a 16 A cube around them (some match,
    some do not) or, for the samples in `far` (entries "r" / "a" per sample index), 100 A away (no match).  cut: per-sample divisor of
    the ligand x receptor search (r = 1), None: r_cross = 7 unscaled.  la_per_atom: capacity of the ligand x atom list per ligand atom;
    ll_short: the ligand list's capacity lies that many entries below its worst case (the packed ligands come within 33 of it)."""
    rng = np.random.default_rng(seed)
    B = len(nl)
    nt = [0] * B if nt is None else nt
    far = dict(far)
    ptr = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int64)       # noqa: E731
    c = SimpleNamespace(B=B, nl=list(nl), nr=list(nr), na=list(na), nt=list(nt), ptr_l=ptr(nl), ptr_r=ptr(nr), ptr_a=ptr(na), ptr_t=ptr(nt),
                        r_lig=r_lig, ll_nb=ll_nb, tor_nb=tor_nb)
    c.Nl, c.Nr, c.Na, c.T = int(sum(nl)), int(sum(nr)), int(sum(na)), int(sum(nt))
    side = r_lig / np.sqrt(3.0) * 0.98
    lp, rp, ap, b0, b1, tp = [], [], [], [], [], []
    for g in range(B):
        centre = rng.uniform(-30, 30, size=3)
        l = centre + rng.uniform(0, side, size=(nl[g], 3))
        lp.append(l)
        for kind, n, dst in (("r", nr[g], rp), ("a", na[g], ap)):
            off = 100.0 if kind in far.get(g, "") else 0.0
            dst.append(centre + off + rng.uniform(-8, 8, size=(n, 3)))
        if bonds and nl[g] > 1:      # a chain, both directions, plus a few extra entries
            i = np.arange(nl[g] - 1)
            e0 = np.concatenate([i, i + 1, rng.integers(0, nl[g], size=3)])
            e1 = np.concatenate([i + 1, i, rng.integers(0, nl[g], size=3)])
            b0.append(e0 + c.ptr_l[g])
            b1.append(e1 + c.ptr_l[g])
        if nt[g]:                     # bond centres: midpoints of ligand atom pairs, some pushed out of reach of part of the ligand
            i, j = rng.integers(0, nl[g], size=nt[g]), rng.integers(0, nl[g], size=nt[g])
            tp.append(0.5 * (l[i] + l[j]) + rng.uniform(-1, 1, size=(nt[g], 3)) * rng.choice([0.0, 4.0], size=(nt[g], 1)))
    cat3 = lambda a: (np.concatenate(a) if a else np.zeros((0, 3))).astype(f32)     # noqa: E731
    c.lpos, c.rpos, c.apos, c.tpos = cat3(lp), cat3(rp), cat3(ap), cat3(tp)
    c.bond0 = np.concatenate(b0).astype(np.int64) if b0 else np.zeros(0, dtype=np.int64)
    c.bond1 = np.concatenate(b1).astype(np.int64) if b1 else np.zeros(0, dtype=np.int64)
    order = rng.permutation(c.bond0.shape[0])           # entry order is arbitrary: not grouped by sample or by node
    c.bond0, c.bond1 = c.bond0[order], c.bond1[order]
    c.Eb = int(c.bond0.shape[0])
    c.max_bonds = max([0] + [int(((c.bond0 >= c.ptr_l[g]) & (c.bond0 < c.ptr_l[g + 1])).sum()) for g in range(B)])
    c.cut = None if cut is None else np.asarray(cut, dtype=f32)
    c.r_cross = 7.0 if cut is None else 1.0
    c.cap_ll = c.Eb + sum(n * min(max(n - 1, 0), ll_nb) for n in nl) - ll_short
    c.cap_lr = sum(a * b for a, b in zip(nl, nr))
    c.cap_la = sum(a * min(b, b if la_per_atom is None else la_per_atom) for a, b in zip(nl, na))
    c.cap_tor = sum(t * min(n, tor_nb) for t, n in zip(nt, nl))
    return c


# id -> arguments of `case`.  Ligand 1 / 3 / 34 / 40 atoms (cap and dropped self pair), receptor 1 / 63 / 64 / 65 / 139 nodes and
# atoms 64 / 65 / 1111 (mask-word and wave boundaries), B = 1 / 2 / 5 with unequal samples, empty lists, capacity overflow,
# with and without a bond prefix, per-sample cutoffs
CASES = {
    "b1_small": dict(seed=1, nl=[3], nr=[1], na=[64], nt=[2], cut=[9.0]),
    "b1_single_atom_no_bonds": dict(seed=2, nl=[1], nr=[63], na=[65], bonds=False),
    "b2_cap_binds": dict(seed=3, nl=[34, 40], nr=[64, 65], na=[65, 64], nt=[5, 0], cut=[8.0, 11.5]),
    "b5_unequal": dict(seed=4, nl=[40, 1, 34, 3, 17], nr=[139, 1, 63, 65, 64], na=[1111, 64, 65, 300, 129], nt=[7, 0, 3, 1, 4],
                       cut=[7.0, 9.5, 12.0, 8.25, 10.0]),
    "b2_one_sample_empty": dict(seed=5, nl=[17, 9], nr=[65, 64], na=[129, 200], nt=[2, 2], far={0: "ra"}, cut=[9.0, 9.0]),
    "b2_all_empty": dict(seed=6, nl=[1, 1], nr=[20, 64], na=[64, 65], far={0: "ra", 1: "ra"}, bonds=False),
    "b2_la_overflow": dict(seed=7, nl=[12, 20], nr=[64, 30], na=[400, 500], nt=[1, 1], la_per_atom=4, cut=[9.0, 10.0]),
    "b3_ll_capacity": dict(seed=9, nl=[12, 36, 9], nr=[20, 64, 5], na=[70, 64, 65], nt=[2, 3, 1], cut=[9.0, 10.0, 8.0], ll_short=150),
    "b1_1111": dict(seed=8, nl=[30], nr=[139], na=[1111], nt=[6], cut=[9.9]),
}
