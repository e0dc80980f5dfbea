"""NumPy float64 restatement of the physics-score guidance term (diffdock_pocket_amd/score_guidance.py states the definition),
independent of the package: nothing here imports it.  It composes the two restatements the tests already have:

    vinardo_ref.score         E = inter + intra of the Vinardo form and g = dE/dx               (step 0 of the definition)
    guidance_ref.direction    d_tr, d_rot, d_tor from x and g                                   (step 2)
    guidance_ref.cap_factor   f = min(1, max_tr / |d32_tr|, max_rot / |d32_rot|, max_tor / max_b |d32_tor[b]|)   (step 3)
    increment = fp32(f * fp64(d32)),  d32 = fp32(w d);  upd = fp32(upd0 + increment)            (step 4)

`forward` returns these with what the bounds and the margins need.  The margins: no typed pair within 1e-6 A of the cutoff, no pair
that a ramp applies to within 1e-6 A of an end of that ramp (the gradient jumps there), and guidance_ref.margins_ok on the
direction (no pair inside the cutoff closer than 1e-3 A: the unit vector of a pair's gradient; bond lengths, lever sums, the inertia
sum)."""
import numpy as np

import guidance_ref as GR
import vinardo_ref as VR

EPS, U24 = GR.EPS, GR.U24


def _pair_margins(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, c):
    """(min_d [S]: the closest pair inside the cutoff, cross or self; ramp_gap: the smallest |s - end| over the pairs inside the
    cutoff that the hydrophobic or the hydrogen-bond ramp applies to and that ramp's two ends)."""
    c = c or VR.DEFAULT
    x = np.asarray(x, np.float64)
    S, n = x.shape[:2]
    rec = np.asarray(rec, np.float64)
    lr, rr = np.asarray(lig_r, np.float64), np.asarray(rec_r, np.float64)
    lf, rf = np.asarray(lig_f).astype(np.int64), np.asarray(rec_f).astype(np.int64)
    min_d, gap = np.full(S, np.inf), np.inf

    def visit(s, d, rsum, ok, fa, fb):
        nonlocal gap
        inside = ok & (d < c.cutoff)
        if not inside.any():
            return
        min_d[s] = min(min_d[s], float(d[inside].min()))
        sd = d - rsum
        hyd = inside & ((fa & fb & 1) != 0)
        hb = inside & (((((fa >> 1) & (fb >> 2)) | ((fa >> 2) & (fb >> 1))) & 1) != 0)
        for sel, ends in ((hyd, (c.hydrophobic_good, c.hydrophobic_bad)), (hb, (c.hbond_good, c.hbond_bad))):
            for end in ends:
                if sel.any():
                    gap = min(gap, float(np.abs(sd[sel] - end).min()))

    for s in range(S):
        if rr.shape[0]:
            r = rec[s] if rec.ndim == 3 else rec
            d = np.sqrt(((x[s][:, None, :] - r[None, :, :]) ** 2).sum(-1))
            visit(s, d, lr[:, None] + rr[None, :], (lr[:, None] >= 0) & (rr[None, :] >= 0), lf[:, None], rf[None, :])
        if pairs is not None and n > 1:
            p = np.triu(np.asarray(pairs), 1).astype(bool)
            d = np.sqrt(((x[s][:, None, :] - x[s][None, :, :]) ** 2).sum(-1))
            visit(s, d, lr[:, None] + lr[None, :], p & (lr[:, None] >= 0) & (lr[None, :] >= 0), lf[:, None], lf[None, :])
    return min_d, gap


def forward(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask, w, caps, upd0=None, c=None):
    """The whole definition for the fp32 weight w.  dict: sc (vinardo_ref.score), eg (e [S, 2] = inter, intra; g; n_pairs, max_term,
    max_grad, min_d: the keys guidance_ref's bounds and margins read), dr (guidance_ref.direction), d32, f, norms, inc (fp32
    increments), upd (fp32, when upd0 = (tr, rot, tor) is given), capped [S] bool, cutoff_gap, ramp_gap."""
    w = float(np.float32(w))
    sc = VR.score(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, 1.0, c)
    min_d, ramp_gap = _pair_margins(x, lig_r, lig_f, rec, rec_r, rec_f, pairs, c)
    eg = dict(e=sc["energy"][:, 4:6].copy(), g=sc["grad"], n_pairs=sc["n_pairs_grad"], max_term=sc["max_term"][:, 4:6].max(1),
              max_grad=sc["max_grad"], min_d=min_d)
    dr = GR.direction(x, eg["g"], bonds, mask)
    d32 = [(w * dr[k]).astype(np.float32) for k in ("d_tr", "d_rot", "d_tor")]
    f, norms = GR.cap_factor(d32, caps)
    inc = [(f[:, None] * v.astype(np.float64)).astype(np.float32) for v in d32]
    out = dict(sc=sc, eg=eg, dr=dr, d32=d32, f=f, norms=norms, inc=inc, capped=f < 1.0, w=w, caps=np.asarray(caps, np.float64),
               cutoff_gap=sc["cutoff_gap"], ramp_gap=ramp_gap)
    if upd0 is not None:
        out["upd"] = [(np.asarray(u, np.float32) + i).astype(np.float32) for u, i in zip(upd0, inc)]
    return out


def margins_ok(ref, n):
    """No pair within 1e-6 of the cutoff or of a ramp end, and the direction margins of guidance_ref.margins_ok."""
    return bool(ref["cutoff_gap"] >= 1e-6) and bool(ref["ramp_gap"] >= 1e-6) and GR.margins_ok(ref, n)


def bounds(ref, n, upd0=None):
    """Error bounds of a comparison against `forward`, two parts composed.
    Energy and gradient: vinardo_ref.bounds, the fp64 summation bound 256 eps (P + 1) max(1, T) - be [S, 2] for (inter, intra) with
    each entry's own pair count and largest weighted pair term, bg [S] with the pairs of either kind and the largest pair gradient.
    Updates: guidance_ref.bounds carries that gradient bound (the same bg: eg holds the pair count and the largest pair gradient it
    is made of) through the ratios of the direction and the cap factor and adds 4 2^-24 (|upd0| + |increment|) per element for the
    fp32 roundings of the definition.
    Returns (be [S, 2], bg [S], [b_tr [S, 3], b_rot [S, 3], b_tor [S, T]])."""
    be7, bg = VR.bounds(ref["sc"])
    _, bg2, bu = GR.bounds(ref, n, upd0)
    assert np.array_equal(bg, bg2)
    return be7[:, 4:6], bg, bu


def random_case(S, n, m, T, seed, per_sample_rec=False, with_pairs=True, caps=(1.0, 0.5, 0.5), c=None):
    """Random poses and receptor atoms in the crowded box of vinardo_ref.random_case (pairs overlap, sit on the ramps and lie outside
    the cutoff; radii from its table with untyped atoms among them on both sides, atom 0 of either always typed; every flag combination 0 .. 7) with the torsions,
    the preloaded updates and the weight of guidance_ref.random_case: T random rotatable bonds with random masks, the last one
    turning only its own end atom (on the axis: exactly 0); the weight chosen from the unweighted direction so that, with S > 1, the
    sample that needs the cap most is capped and the one that needs it least is not (S = 1: capped for even seeds, uncapped for odd
    ones).  Redrawn (seed + 7919 k) until margins_ok holds.  Returns a dict of fp32 / integer arrays, the weight, the caps, upd0 and
    ref = forward."""
    assert T == 0 or n >= 2
    caps = np.asarray(caps, np.float64)
    table = np.array(list(VR.RADII.values()) + [-1.0, -1.0], dtype=np.float32)
    for k in range(64):
        rng = np.random.default_rng(seed + 7919 * k)
        box = 1.6 * max(n, 8) ** (1 / 3)
        x = (rng.standard_normal((S, n, 3)) * box).astype(np.float32)
        rec = (rng.standard_normal(((S, m, 3) if per_sample_rec else (m, 3))) * box).astype(np.float32)
        lig_r, rec_r = table[rng.integers(0, len(table), n)], table[rng.integers(0, len(table), m)]
        lig_f, rec_f = rng.integers(0, 8, n).astype(np.uint8), rng.integers(0, 8, m).astype(np.uint8)
        lig_r[0] = table[rng.integers(0, len(table) - 2)]        # atom 0 of either side is typed: one atom does take part
        if m:
            rec_r[0] = table[rng.integers(0, len(table) - 2)]
        pairs = np.triu(rng.random((n, n)) < 0.5, 1).astype(np.uint8) if with_pairs else None
        bonds = np.stack([rng.permutation(n)[:2] for _ in range(T)]).astype(np.int64) if T else np.zeros((0, 2), np.int64)
        mask = rng.random((T, n)) < 0.4
        if T > 1:
            mask[-1] = False
            mask[-1, bonds[-1, 0]] = True
        upd0 = [rng.standard_normal((S, 3)).astype(np.float32), (0.3 * rng.standard_normal((S, 3))).astype(np.float32),
                (0.3 * rng.standard_normal((S, T))).astype(np.float32)]
        args = (x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask)
        unit = forward(*args, 1.0, (np.inf, np.inf, np.inf), c=c)
        need = (unit["norms"] / caps[None, :]).max(1)            # capped iff w * need > 1
        pos = np.sort(need[need > 0])
        if len(pos) == 0:
            w = 1.0
        elif S == 1 or pos[0] == pos[-1]:
            w = (2.0 if seed % 2 == 0 else 0.5) / pos[-1]
        else:
            w = 1.0 / np.sqrt(pos[0] * pos[-1])
        w = float(np.float32(w))
        ref = forward(*args, w, caps, upd0, c=c)
        if margins_ok(ref, n):
            return dict(x=x, lig_r=lig_r, lig_f=lig_f, rec=rec, rec_r=rec_r, rec_f=rec_f, pairs=pairs, bonds=bonds, mask=mask, w=w,
                        caps=caps, upd0=upd0, ref=ref, need=need)
    raise AssertionError("no draw keeps the margins")


rel_dev = GR.rel_dev
