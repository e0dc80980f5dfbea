"""An independent NumPy fp64 restatement of the Vinardo-form score (the definition in the docstring of diffdock_pocket_amd/scoring.py),
for the tests of the PyTorch form and of csrc/ddp_score.hip.  It imports nothing from the package: the constants are written out
again here, every pair term is kept apart, and what the error bound needs (the number of pairs inside the cutoff, the largest pair
term of every entry, the largest pair gradient, the closest approach of any pair to the cutoff) is returned with the result.

    pair (i, j), both radii >= 0, d < cutoff (strict), s = d - R_i - R_j
    gauss = exp(-(s / 0.8)^2)    repulsion = s^2 [s < 0]
    hydrophobic [both bit 0] = 1 (s <= 0), (2.5 - s) / 2.5 (s < 2.5), 0
    hbond [bit 1 of one and bit 2 of the other] = 1 (s <= -0.6), -s / 0.6 (s < 0), 0
    inter = -0.045 G + 0.8 R - 0.035 H - 0.6 B,  intra: the same over the self pairs,  total = inter / tor_divisor
    grad_i = d(inter + intra)/dx_i; the ramps' slopes on the open intervals only; d = 0: no gradient

The numbers above are the defaults.  Every function takes an optional `c`, a Constants, for another set of the eleven:
    gauss = exp(-((s - gauss_offset) / gauss_width)^2),  a ramp = 1 (s <= good), (bad - s) / (bad - good) (s < bad), 0"""
import collections

import numpy as np

CUTOFF = 8.0
GAUSS_WIDTH = 0.8
HYDROPHOBIC_BAD = 2.5
HBOND_GOOD = -0.6
WEIGHTS = np.array([-0.045, 0.8, -0.035, -0.6])
W_TORSION = 0.0585
RADII = {"C": 2.0, "N": 1.75, "O": 1.6, "P": 2.1, "S": 2.0, "F": 1.545, "Cl": 2.045, "Br": 2.165, "I": 2.36}
EPS = 2.0 ** -53
Constants = collections.namedtuple("Constants", ["cutoff", "gauss_offset", "gauss_width", "hydrophobic_good", "hydrophobic_bad", "hbond_good",
                                                 "hbond_bad", "w_gauss", "w_repulsion", "w_hydrophobic", "w_hbond"])
DEFAULT = Constants(CUTOFF, 0.0, GAUSS_WIDTH, 0.0, HYDROPHOBIC_BAD, HBOND_GOOD, 0.0, *WEIGHTS)


def weights(c=None):
    """[w_gauss, w_repulsion, w_hydrophobic, w_hbond] of the constants c."""
    c = c or DEFAULT
    return np.array([c.w_gauss, c.w_repulsion, c.w_hydrophobic, c.w_hbond])


def pair_terms(diff, rsum, fa, fb, c=None):
    """diff [P, 3] (first - second), rsum [P], flag bytes fa, fb [P] of pairs of typed atoms -> (inside [P] bool, terms [P, 4] (zero
    outside the cutoff), dE/d(first atom) [P, 3] of the weighted pair energy, d [P]).  c: the constants (None: the defaults)."""
    c = c or DEFAULT
    diff = np.asarray(diff, dtype=np.float64)
    d = np.sqrt((diff ** 2).sum(-1))
    with np.errstate(invalid="ignore"):
        inside = ~(d >= c.cutoff)                   # a NaN distance is inside: it poisons the sums
        s = d - rsum
        t = np.zeros((len(d), 4))
        de = np.zeros((len(d), 4))                 # d term / d s
        ga = np.exp(-((s - c.gauss_offset) / c.gauss_width) ** 2)
        t[:, 0] = ga
        de[:, 0] = ga * (-2.0 * (s - c.gauss_offset) / c.gauss_width ** 2)
        t[:, 1] = np.where(s < 0, s * s, 0.0)
        de[:, 1] = np.where(s < 0, 2.0 * s, 0.0)
        hyd = ((fa & fb & 1) != 0)
        good, bad = c.hydrophobic_good, c.hydrophobic_bad
        t[:, 2] = np.where(hyd, np.where(s <= good, 1.0, np.where(s < bad, (bad - s) / (bad - good), 0.0)), 0.0)
        de[:, 2] = np.where(hyd & (s > good) & (s < bad), -1.0 / (bad - good), 0.0)
        hb = ((((fa >> 1) & (fb >> 2)) | ((fa >> 2) & (fb >> 1))) & 1) != 0
        good, bad = c.hbond_good, c.hbond_bad
        t[:, 3] = np.where(hb, np.where(s <= good, 1.0, np.where(s < bad, (bad - s) / (bad - good), 0.0)), 0.0)
        de[:, 3] = np.where(hb & (s > good) & (s < bad), -1.0 / (bad - good), 0.0)
        t[~inside] = 0.0
        de[~inside] = 0.0
        unit = np.where((d != 0)[:, None], diff / np.where(d != 0, d, 1.0)[:, None], 0.0)
    return inside, t, (de @ weights(c))[:, None] * unit, d


def score(x, lig_r, lig_f, rec, rec_r, rec_f, pairs=None, tor_divisor=1.0, c=None):
    """x [S, n, 3], rec [m, 3] or [S, m, 3] (any float type: converted to fp64 first), radii (negative: untyped), uint8 flags, pairs
    uint8 [n, n] upper triangle or None.  Returns a dict:
      energy [S, 7], grad [S, n, 3]
      n_pairs [S, 7]: pairs inside the cutoff behind every energy entry (ligand-receptor for all but entry 5, the self pairs there)
      max_term [S, 7]: the largest |pair term| of every entry (weighted for inter / intra / total)
      n_pairs_grad [S], max_grad [S]: pairs inside the cutoff of either kind, the largest pair gradient norm
      cutoff_gap: min over all typed pairs met of |d - cutoff|.
    c: the constants (None: the defaults)."""
    c = c or DEFAULT
    WEIGHTS, CUTOFF = weights(c), c.cutoff
    x = np.asarray(x, dtype=np.float64)
    S, n = x.shape[:2]
    rec = np.asarray(rec, dtype=np.float64)
    lig_r, rec_r = np.asarray(lig_r, dtype=np.float64), np.asarray(rec_r, dtype=np.float64)
    lig_f, rec_f = np.asarray(lig_f).astype(np.int64), np.asarray(rec_f).astype(np.int64)
    li, rj = np.nonzero(lig_r >= 0)[0], np.nonzero(rec_r >= 0)[0]
    ci, cj = (a.reshape(-1) for a in np.meshgrid(li, rj, indexing="ij"))
    if pairs is not None:
        pi, pj = np.nonzero(np.triu(np.asarray(pairs), 1))
        ok = (lig_r[pi] >= 0) & (lig_r[pj] >= 0)
        pi, pj = pi[ok], pj[ok]
    else:
        pi = pj = np.zeros(0, dtype=np.int64)
    out = {"energy": np.zeros((S, 7)), "grad": np.zeros((S, n, 3)), "n_pairs": np.zeros((S, 7)), "max_term": np.zeros((S, 7)),
           "n_pairs_grad": np.zeros(S), "max_grad": np.zeros(S), "cutoff_gap": np.inf}
    for s in range(S):
        r = rec[s] if rec.ndim == 3 else rec
        e, g = out["energy"][s], out["grad"][s]
        inside, t, pg, d = pair_terms(x[s, ci] - r[cj], lig_r[ci] + rec_r[cj], lig_f[ci], rec_f[cj], c)
        e[:4] = t.sum(0)
        e[4] = WEIGHTS @ e[:4]
        np.add.at(g, ci, pg)
        w = t @ WEIGHTS
        out["n_pairs"][s, [0, 1, 2, 3, 4, 6]] = inside.sum()
        if len(d):
            out["max_term"][s, :4] = np.abs(t).max(0)
            out["max_term"][s, 4] = np.abs(w).max()
            out["max_term"][s, 6] = np.abs(w).max() / tor_divisor
            out["max_grad"][s] = np.sqrt((pg ** 2).sum(-1)).max()
            out["cutoff_gap"] = min(out["cutoff_gap"], np.nanmin(np.abs(d - CUTOFF)) if np.isfinite(d).any() else np.inf)
        out["n_pairs_grad"][s] = inside.sum()
        if len(pi):
            inside, t, pg, d = pair_terms(x[s, pi] - x[s, pj], lig_r[pi] + lig_r[pj], lig_f[pi], lig_f[pj], c)
            w = t @ WEIGHTS
            e[5] = WEIGHTS @ t.sum(0)
            np.add.at(g, pi, pg)
            np.add.at(g, pj, -pg)
            out["n_pairs"][s, 5] = inside.sum()
            out["max_term"][s, 5] = np.abs(w).max()
            out["max_grad"][s] = max(out["max_grad"][s], np.sqrt((pg ** 2).sum(-1)).max())
            out["n_pairs_grad"][s] += inside.sum()
            out["cutoff_gap"] = min(out["cutoff_gap"], np.nanmin(np.abs(d - CUTOFF)) if np.isfinite(d).any() else np.inf)
        e[6] = e[4] / tor_divisor
    return out


def bounds(ref):
    """The error bound of a comparison against `score`: per energy entry 256 2^-53 (P + 1) max(1, largest |pair term| of that entry), P
    the pairs inside the cutoff; per gradient component the same with the largest pair gradient norm.  Both sides sum the same fp64
    pair terms (each within a few ulp of the other side's: sqrt, exp and the divisions are correctly rounded or within 1-2 ulp) in
    different orders: the sum of P terms of size <= T is off by at most P eps (P T) in the worst case and by about sqrt(P) eps T for
    the blocked sums used here; 256 (P + 1) eps max(1, T) sits between the two and is what the issue sets.
    Returns (energy bound [S, 7], gradient bound [S])."""
    be = 256.0 * EPS * (ref["n_pairs"] + 1.0) * np.maximum(1.0, ref["max_term"])
    bg = 256.0 * EPS * (ref["n_pairs_grad"] + 1.0) * np.maximum(1.0, ref["max_grad"])
    return be, bg


def random_case(S, n, m, seed, per_sample_rec=False, with_pairs=True, c=None):
    """Random poses in a box crowded enough that pairs overlap, sit on the ramps and lie outside the cutoff; radii from the table with
    untyped atoms (-1: hydrogens, metals) among them on both sides; every flag combination 0 .. 7.  Redrawn (seed + 7919 k) until the
    reference meets no pair within 1e-6 of the cutoff, the only discontinuity.  fp32 inputs as the package takes them; returns
    (x, lig_r, lig_f, rec, rec_r, rec_f, pairs or None, ref of score()).  c: the constants of that reference (None: the defaults)."""
    table = np.array(list(RADII.values()) + [-1.0, -1.0], dtype=np.float32)
    for k in range(64):
        rng = np.random.default_rng(seed + 7919 * k)
        box = 1.6 * max(n, 8) ** (1 / 3)
        x = (rng.standard_normal((S, n, 3)) * box).astype(np.float32)
        rec = (rng.standard_normal(((S, m, 3) if per_sample_rec else (m, 3))) * box).astype(np.float32)
        lig_r, rec_r = table[rng.integers(0, len(table), n)], table[rng.integers(0, len(table), m)]
        lig_f, rec_f = rng.integers(0, 8, n).astype(np.uint8), rng.integers(0, 8, m).astype(np.uint8)
        pairs = np.triu(rng.random((n, n)) < 0.5, 1).astype(np.uint8) if with_pairs else None
        ref = score(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, 1.0 + W_TORSION * 3, c)
        if ref["cutoff_gap"] >= 1e-6:
            return x, lig_r, lig_f, rec, rec_r, rec_f, pairs, ref
    raise AssertionError("no draw clear of the cutoff")
