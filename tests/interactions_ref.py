"""An independent NumPy fp64 restatement of the per-residue interaction profile (the definition in the docstring of
diffdock_pocket_amd/interactions.py), for the tests of the PyTorch form and of csrc/ddp_profile.hip.  It imports nothing from the
package; the pair terms are those of tests/vinardo_ref.py, kept apart pair by pair, and what the error bound needs (the number of
pairs inside the cutoff and the largest pair term of every entry) and what the bit comparison needs (the closest approach of any
typed pair to one of the thresholds) is returned with the result.

    residue r owns the receptor atoms res_ptr[r] .. res_ptr[r + 1] - 1; pairs (i, j in r), both radii >= 0, d < 8 (strict)
    terms = the four sums of vinardo_ref.pair_terms, energy = WEIGHTS . terms, pairs = their number, d_min = the smallest d (+inf: none)
    bits: 1 CONTACT iff d_min < contact_distance, 2 HYDROPHOBIC iff terms[2] > 0, 4 HBOND iff terms[3] > 0
    poison: a non-finite coordinate of a typed ligand atom -> every residue of the sample; of a typed atom of residue r -> that residue
    of the sample; a poisoned entry: terms, energy, d_min NaN, pairs 0, bits 0"""
import numpy as np

from vinardo_ref import DEFAULT, EPS, RADII, pair_terms, weights

CONTACT_DISTANCE = 4.5


def profile(x, lig_r, lig_f, rec, rec_r, rec_f, res_ptr, contact_distance=CONTACT_DISTANCE, c=None):
    """x [S, n, 3], rec [m, 3] or [S, m, 3] (any float type: converted to fp64 first), radii (negative: untyped), uint8 flags, res_ptr
    [R + 1].  Returns a dict:
      terms [S, R, 4], energy [S, R], d_min [S, R], pairs [S, R] (int64), bits [S, R] (uint8)
      max_term [S, R, 5]: the largest |pair term| behind terms[..., k] and (last) behind energy, weighted
      grad_l1 [S, R]: the sum over the entry's pairs of the 1-norm of the pair energy's gradient: what a unit shift of every coordinate
      can move `energy` by, to first order
      gap [S]: per sample, the smallest of |d - cutoff|, |d - contact_distance| over all typed pairs, |s - 2.5| over the hydrophobic
      pairs and |s - 0| over the donor-acceptor pairs (the thresholds are the only discontinuities); threshold_gap: its minimum.
    c: a vinardo_ref.Constants (None: the defaults, to which the numbers above belong; the thresholds follow c: cutoff,
    hydrophobic_bad, hbond_bad)."""
    c = c or DEFAULT
    WEIGHTS, CUTOFF, HYDROPHOBIC_BAD, HBOND_BAD = weights(c), c.cutoff, c.hydrophobic_bad, c.hbond_bad
    x = np.asarray(x, dtype=np.float64)
    S = x.shape[0]
    rec = np.asarray(rec, dtype=np.float64)
    lig_r, rec_r = np.asarray(lig_r, dtype=np.float64), np.asarray(rec_r, dtype=np.float64)
    lig_f, rec_f = np.asarray(lig_f).astype(np.int64), np.asarray(rec_f).astype(np.int64)
    ptr = np.asarray(res_ptr, dtype=np.int64)
    R = len(ptr) - 1
    li = np.nonzero(lig_r >= 0)[0]
    out = {"terms": np.zeros((S, R, 4)), "energy": np.zeros((S, R)), "d_min": np.full((S, R), np.inf), "pairs": np.zeros((S, R), dtype=np.int64),
           "bits": np.zeros((S, R), dtype=np.uint8), "max_term": np.zeros((S, R, 5)), "grad_l1": np.zeros((S, R)), "gap": np.full(S, np.inf)}
    for s in range(S):
        r = rec[s] if rec.ndim == 3 else rec
        lig_bad = not np.isfinite(x[s, li]).all()
        for k in range(R):
            rj = np.arange(ptr[k], ptr[k + 1])
            rj = rj[rec_r[rj] >= 0]
            if lig_bad or not np.isfinite(r[rj]).all():
                out["terms"][s, k], out["energy"][s, k], out["d_min"][s, k] = np.nan, np.nan, np.nan
                continue
            ci, cj = (a.reshape(-1) for a in np.meshgrid(li, rj, indexing="ij"))
            if len(ci) == 0:
                continue
            inside, t, pg, d = pair_terms(x[s, ci] - r[cj], lig_r[ci] + rec_r[cj], lig_f[ci], rec_f[cj], c)
            out["terms"][s, k] = t.sum(0)
            out["energy"][s, k] = WEIGHTS @ out["terms"][s, k]
            out["pairs"][s, k] = inside.sum()
            out["max_term"][s, k, :4] = np.abs(t).max(0)
            out["max_term"][s, k, 4] = np.abs(t @ WEIGHTS).max()
            out["grad_l1"][s, k] = np.abs(pg).sum()
            if inside.any():
                out["d_min"][s, k] = d[inside].min()
            out["bits"][s, k] = (1 if out["d_min"][s, k] < contact_distance else 0) | (2 if out["terms"][s, k, 2] > 0 else 0) \
                | (4 if out["terms"][s, k, 3] > 0 else 0)
            sd = d - (lig_r[ci] + rec_r[cj])
            hyd = (lig_f[ci] & rec_f[cj] & 1) != 0
            hb = ((((lig_f[ci] >> 1) & (rec_f[cj] >> 2)) | ((lig_f[ci] >> 2) & (rec_f[cj] >> 1))) & 1) != 0
            gaps = [np.abs(d - CUTOFF).min(), np.abs(d - contact_distance).min()]
            if hyd.any():
                gaps.append(np.abs(sd[hyd] - HYDROPHOBIC_BAD).min())
            if hb.any():
                gaps.append(np.abs(sd[hb] - HBOND_BAD).min())
            out["gap"][s] = min(out["gap"][s], min(gaps))
    out["threshold_gap"] = float(out["gap"].min()) if S else np.inf
    return out


def bounds(ref):
    """vinardo_ref.bounds applied per residue: 256 2^-53 (pairs + 1) max(1, largest |pair term| of that entry).
    Returns (terms bound [S, R, 4], energy bound [S, R])."""
    b = 256.0 * EPS * (ref["pairs"][..., None] + 1.0) * np.maximum(1.0, ref["max_term"])
    return b[..., :4], b[..., 4]


D_MIN_RTOL = 8.0 * EPS      # d^2 with or without FMA (three products, two additions), then a correctly rounded sqrt


def check(got_terms, got_energy, got_d_min, got_pairs, got_bits, ref, what="", bits_where=None):
    """A profile (arrays shaped as in `profile`) against the restatement: terms and energy within `bounds`, d_min within D_MIN_RTOL
    relative (inf and NaN have to match), pairs and bits exactly (bits_where [S] bool: only in these samples).  NaN has to sit exactly
    where the restatement has it.  Prints the worst ratio."""
    bt, be = bounds(ref)
    gt, ge, gd = np.asarray(got_terms), np.asarray(got_energy), np.asarray(got_d_min)
    nan = np.isnan(ref["energy"])
    assert np.array_equal(np.isnan(ge), nan) and np.array_equal(np.isnan(gd), nan) and np.array_equal(np.isnan(gt).any(-1), nan), what
    assert np.array_equal(np.isnan(gt).all(-1), nan), what
    ok = ~nan
    et, ee = np.abs(gt - ref["terms"])[ok], np.abs(ge - ref["energy"])[ok]
    if ok.any():
        print(what, "terms worst |err| / bound:", float((et / bt[ok]).max()), "energy:", float((ee / be[ok]).max()))
    assert (et <= bt[ok]).all() and (ee <= be[ok]).all(), what
    rd = ref["d_min"][ok]
    fin = np.isfinite(rd)
    assert np.array_equal(np.isfinite(gd[ok]), fin), what
    assert (np.abs(gd[ok][fin] - rd[fin]) <= D_MIN_RTOL * rd[fin]).all(), what
    assert np.array_equal(np.asarray(got_pairs), ref["pairs"]), what
    gb = np.asarray(got_bits)
    if bits_where is None:
        assert np.array_equal(gb, ref["bits"]), what
    else:
        assert np.array_equal(gb[bits_where], ref["bits"][bits_where]), what


def random_case(S, n, sizes, seed, per_sample_rec=False, untyped_residue=None, ligand_untyped=False, contact_distance=CONTACT_DISTANCE,
                c=None):
    """Random poses and a receptor of residues with the given sizes (atoms per residue, zeros allowed), drawn as
    vinardo_ref.random_case draws them: a box crowded enough that pairs overlap, sit on the ramps and lie outside the cutoff; radii from
    the table with untyped atoms (-1) among them; every flag combination 0 .. 7.  With two or more atoms on a side, one of them is
    made untyped whatever the draw gave (the last ligand atom, the first receptor atom); untyped_residue: that residue's atoms are all
    untyped; ligand_untyped: every ligand atom is.  Redrawn (seed + 7919 k) until no typed pair lies within 1e-6 of a threshold;
    raises after 64 draws.  fp32 inputs as the package takes them; returns (x, lig_r, lig_f, rec, rec_r, rec_f, res_ptr, ref).  c: the
    constants of that reference (None: the defaults)."""
    table = np.array(list(RADII.values()) + [-1.0, -1.0], dtype=np.float32)
    sizes = np.asarray(sizes, dtype=np.int64)
    m = int(sizes.sum())
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    for k in range(64):
        rng = np.random.default_rng(seed + 7919 * k)
        box = 1.6 * max(n, 8) ** (1 / 3)
        x = (rng.standard_normal((S, n, 3)) * box).astype(np.float32)
        rec = (rng.standard_normal(((S, m, 3) if per_sample_rec else (m, 3))) * box).astype(np.float32)
        lig_r, rec_r = table[rng.integers(0, len(table), n)], table[rng.integers(0, len(table), m)]
        lig_f, rec_f = rng.integers(0, 8, n).astype(np.uint8), rng.integers(0, 8, m).astype(np.uint8)
        if n >= 2:
            lig_r[n - 1] = -1.0
        if m >= 2:
            rec_r[0] = -1.0
        if untyped_residue is not None:
            rec_r[ptr[untyped_residue]:ptr[untyped_residue + 1]] = -1.0
        if ligand_untyped:
            lig_r[:] = -1.0
        ref = profile(x, lig_r, lig_f, rec, rec_r, rec_f, ptr, contact_distance, c)
        if ref["threshold_gap"] >= 1e-6:
            return x, lig_r, lig_f, rec, rec_r, rec_f, ptr, ref
    raise AssertionError("no draw clear of the thresholds")
