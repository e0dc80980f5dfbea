"""NumPy float64 restatement of the steric-clash guidance term (diffdock_pocket_amd/guidance.py states the definition), independent
of the package: nothing here imports it.  For fp32 poses x [S, n, 3], radii, a receptor [m, 3] (shared) or [S, m, 3] (per sample; a
negative radius = a hydrogen, ignored), self_pairs [n, n] (upper triangle) or None, rotatable bonds [T, 2] = (u, v) with
mask_rotate [T, n]:

    t_ij = r_i + r_j - 2 overlap (a pair with t_ij <= 0 never counts),  E = sum max(0, t_ij - d_ij)^2 over cross and self pairs
    g = dE/dx;  d_tr = -sum g_i / n;  d_rot = -sum (x_i - c) x g_i / sum |x_i - c|^2;
    d_tor[b] = -sum g_i . a_i / sum |a_i|^2,  a_i = u^ x (x_i - x_v) over mask_rotate[b] without u and v;  a zero denominator gives 0
    d32 = fp32(w d);  f = min(1, max_tr / |d32_tr|, max_rot / |d32_rot|, max_tor / max_b |d32_tor[b]|) (zero norms: no constraint)
    increment = fp32(f * fp64(d32));  upd = fp32(upd0 + increment)

`forward` returns these together with what the error bounds and the margins need."""
import numpy as np

EPS = 2.0 ** -53
U24 = 2.0 ** -24
OVERLAP = 0.4
RADII = np.array([1.7, 1.55, 1.52, 1.8, 1.47, 1.75, 1.2], dtype=np.float32)       # C N O S F Cl and a small one


def energy_grad(x, lig_r, rec, rec_r, pairs, overlap=OVERLAP):
    """dict: e [S, 2] = (E_cross, E_self), g [S, n, 3], and per sample n_pairs (pairs with a positive penalty; a self pair counts once
    per end, as it is summed), max_term (largest energy term), max_grad (largest norm of a pair's gradient), min_d (closest such
    pair)."""
    x = np.asarray(x, np.float64)
    S, n = x.shape[:2]
    r = np.asarray(lig_r, np.float64)
    rr = np.asarray(rec_r, np.float64)
    m = rr.shape[0]
    out = dict(e=np.zeros((S, 2)), g=np.zeros((S, n, 3)), n_pairs=np.zeros(S), max_term=np.zeros(S), max_grad=np.zeros(S),
               min_d=np.full(S, np.inf))
    t_c = r[:, None] + rr[None, :] - 2.0 * overlap
    ok_c = (rr[None, :] >= 0) & (t_c > 0)
    t_s = r[:, None] + r[None, :] - 2.0 * overlap
    ok_s = None
    if pairs is not None:
        p = np.asarray(pairs).astype(bool)
        ok_s = (p | p.T) & (t_s > 0) & ~np.eye(n, dtype=bool)

    def terms(diff, t, ok, s, col, half):
        d = np.sqrt((diff * diff).sum(-1))
        pen = np.where(ok, np.maximum(t - d, 0.0), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            unit = np.where((d > 0)[..., None], diff / d[..., None], 0.0)
        gp = (-2.0 * pen)[..., None] * unit
        out["e"][s, col] = (0.5 if half else 1.0) * (pen * pen).sum()
        out["g"][s] += gp.sum(1)
        hit = pen > 0
        out["n_pairs"][s] += hit.sum()
        if hit.any():
            out["max_term"][s] = max(out["max_term"][s], float((pen * pen).max()))
            out["max_grad"][s] = max(out["max_grad"][s], float(np.sqrt((gp * gp).sum(-1)).max()))
            out["min_d"][s] = min(out["min_d"][s], float(d[hit].min()))

    for s in range(S):
        if m > 0:
            rs = np.asarray(rec[s] if np.ndim(rec) == 3 else rec, np.float64)
            terms(x[s][:, None, :] - rs[None, :, :], t_c, ok_c, s, 0, False)
        if ok_s is not None:
            terms(x[s][:, None, :] - x[s][None, :, :], t_s, ok_s, s, 1, True)
    return out


def direction(x, g, bonds, mask):
    """dict: the unweighted d_tr [S, 3], d_rot [S, 3], d_tor [S, T]; the margins bond_len [S, T], den_tor [S, T], den_rot [S]; and the
    magnitudes the bounds take: p_max [S] (largest |x_i - c|), lever_max [S, T], count [T] (atoms in a bond's sums)."""
    x = np.asarray(x, np.float64)
    S, n = x.shape[:2]
    bonds = np.asarray(bonds, np.int64).reshape(-1, 2)
    T = bonds.shape[0]
    mask = np.asarray(mask).astype(bool).reshape(T, n)
    c = x.mean(1, keepdims=True)
    p = x - c
    den_rot = (p * p).sum((1, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        d_rot = np.where(den_rot[:, None] == 0, 0.0, -np.cross(p, g).sum(1) / den_rot[:, None])
    out = dict(d_tr=-g.sum(1) / n, d_rot=d_rot, d_tor=np.zeros((S, T)), bond_len=np.zeros((S, T)), den_tor=np.zeros((S, T)),
               den_rot=den_rot, p_max=np.sqrt((p * p).sum(-1)).max(1), lever_max=np.zeros((S, T)), count=np.zeros(T))
    for b in range(T):
        u, v = bonds[b]
        mk = mask[b].copy()
        mk[u] = mk[v] = False
        axis = x[:, u] - x[:, v]
        ln = np.sqrt((axis * axis).sum(-1))
        out["bond_len"][:, b] = ln
        out["count"][b] = mk.sum()
        if not mk.any():
            continue
        a = np.cross((axis / ln[:, None])[:, None, :], x[:, mk] - x[:, v][:, None, :])
        num, den = (g[:, mk] * a).sum((1, 2)), (a * a).sum((1, 2))
        out["den_tor"][:, b] = den
        out["lever_max"][:, b] = np.sqrt((a * a).sum(-1)).max(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["d_tor"][:, b] = np.where(den == 0, 0.0, -num / den)
    return out


def cap_factor(d32, caps):
    """f [S] float64 from the fp32 direction d32 = (tr, rot, tor) and caps = (max_tr, max_rot, max_tor); norms [S, 3]."""
    S = d32[0].shape[0]
    tor = np.abs(d32[2].astype(np.float64)).max(1) if d32[2].shape[1] else np.zeros(S)
    norms = np.stack([np.sqrt((d32[0].astype(np.float64) ** 2).sum(1)), np.sqrt((d32[1].astype(np.float64) ** 2).sum(1)), tor], 1)
    f = np.ones(S)
    for k in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(norms[:, k] > 0, np.minimum(f, caps[k] / norms[:, k]), f)
    return f, norms


def forward(x, lig_r, rec, rec_r, pairs, bonds, mask, w, caps, upd0=None, overlap=OVERLAP):
    """The whole definition for the fp32 weight w.  dict: eg (energy_grad), dr (direction), d32, f, norms, inc (fp32 increments), upd
    (fp32, when upd0 = (tr, rot, tor) is given), capped [S] bool."""
    w = float(np.float32(w))
    eg = energy_grad(x, lig_r, rec, rec_r, pairs, overlap)
    dr = direction(x, eg["g"], bonds, mask)
    d32 = [(w * dr[k]).astype(np.float32) for k in ("d_tr", "d_rot", "d_tor")]
    f, norms = cap_factor(d32, caps)
    inc = [(f[:, None] * v.astype(np.float64)).astype(np.float32) for v in d32]
    out = dict(eg=eg, dr=dr, d32=d32, f=f, norms=norms, inc=inc, capped=f < 1.0, w=w, caps=np.asarray(caps, np.float64))
    if upd0 is not None:
        out["upd"] = [(np.asarray(u, np.float32) + i).astype(np.float32) for u, i in zip(upd0, inc)]
    return out


def margins_ok(ref, n):
    """The inequalities every case has to keep, in float64: no counted pair closer than 1e-3 A, every rotatable bond longer than 0.1 A
    with lever sum den > 1e-6 (a bond that turns no atom off its axis has den = 0 exactly and gives 0: not a margin case), and for
    n > 1 sum |x - c|^2 > 1e-6."""
    dr = ref["dr"]
    ok = bool((ref["eg"]["min_d"] >= 1e-3).all())
    turning = dr["count"] > 0
    ok &= bool((dr["bond_len"] > 0.1).all()) and bool((dr["den_tor"][:, turning] > 1e-6).all())
    if n > 1:
        ok &= bool((dr["den_rot"] > 1e-6).all())
    return ok


def bounds(ref, n, upd0=None):
    """Error bounds of a comparison against `forward`.
    Energy and gradient (both sides sum the same fp64 pair terms in different orders), in the form of vinardo_ref.bounds:
        be [S] = 256 eps (P + 1) max(1, largest energy term),   bg [S] = 256 eps (P + 1) max(1, largest pair gradient norm)
    carried through the ratios of the direction: a sum of k terms, each a product of a gradient component (error bg) with a lever of
    size <= L, is off by at most k c L bg from its inputs (c = 1 translation, 2 cross product, 3 dot product with a_i) plus
    256 eps (k + 1) max(1, largest term) from its own summation; a denominator sum |.|^2 of k positive terms is off by at most
    256 eps (k + 1) relative; num / den inherits d_num / den + |num / den| d_den.  Times w: the bound of the unrounded direction.  The
    cap factor is a continuous function of the norms: its relative error is at most the largest relative error of a norm that can
    bind (cap / norm <= 1 + 1e-6).  On top, the fp32 roundings of the definition (direction, increment, sum):
        4 2^-24 (|upd0| + |increment|) per element.
    Returns (be [S], bg [S], [b_tr [S, 3], b_rot [S, 3], b_tor [S, T]])."""
    eg, dr, w = ref["eg"], ref["dr"], ref["w"]
    P = eg["n_pairs"]
    be = 256.0 * EPS * (P + 1.0) * np.maximum(1.0, eg["max_term"])
    bg = 256.0 * EPS * (P + 1.0) * np.maximum(1.0, eg["max_grad"])
    gmax = np.abs(eg["g"]).max((1, 2))
    own = 256.0 * EPS * (n + 1.0)
    b_tr = w * (n * bg + own * np.maximum(1.0, gmax)) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        L = dr["p_max"]
        b_rot = np.where(dr["den_rot"] > 0, w * ((n * 2.0 * L * bg + own * np.maximum(1.0, 2.0 * L * gmax)) / dr["den_rot"]
                                                 + np.abs(dr["d_rot"]).max(1) * own), 0.0)
        k = dr["count"][None, :]
        Lt = dr["lever_max"]
        ownk = 256.0 * EPS * (k + 1.0)
        b_tor = np.where(dr["den_tor"] > 0, w * ((k * 3.0 * Lt * bg[:, None] + ownk * np.maximum(1.0, 3.0 * Lt * gmax[:, None])) / dr["den_tor"]
                                                 + np.abs(dr["d_tor"]) * ownk), 0.0)
    b_dir = [np.repeat(b_tr[:, None], 3, 1), np.repeat(b_rot[:, None], 3, 1), b_tor]
    caps_norm_err = np.stack([np.sqrt(3.0) * b_tr, np.sqrt(3.0) * b_rot, b_tor.max(1) if b_tor.shape[1] else np.zeros_like(b_tr)], 1)
    norms = ref["norms"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(norms > 0, caps_norm_err / norms, 0.0)
        binding = np.where(norms > 0, ref["caps"][None, :] / norms <= 1.0 + 1e-6, False)
    relf = np.where(binding, rel, 0.0).max(1)
    out = []
    for j in range(3):
        inc = np.abs(ref["inc"][j].astype(np.float64))
        u0 = np.abs(np.asarray(upd0[j], np.float64)) if upd0 is not None else 0.0
        out.append(b_dir[j] + inc * relf[:, None] + 4.0 * U24 * (u0 + inc))
    return be, bg, out


def random_case(S, n, m, T, seed, per_sample_rec=False, with_pairs=True, caps=(1.0, 0.5, 0.5)):
    """Random poses and receptor atoms in a box crowded enough that pairs overlap; ligand radii from RADII, receptor radii from RADII
    with hydrogens (-1) among them; T random rotatable bonds with random masks, the last one turning only its own end atom (on the
    axis: exactly 0).  The weight is chosen from the unweighted direction so that, with S > 1, the sample that needs the cap most is
    capped and the one that needs it least is not (S = 1: capped for even seeds, uncapped for odd ones).  Redrawn (seed + 7919 k)
    until margins_ok holds.  Returns a dict of fp32 / integer arrays, the weight, the caps, upd0 (random preload) and ref = forward."""
    assert T == 0 or n >= 2
    caps = np.asarray(caps, np.float64)
    for k in range(64):
        rng = np.random.default_rng(seed + 7919 * k)
        box = 1.6 * max(n, 8) ** (1 / 3)
        x = (rng.standard_normal((S, n, 3)) * box).astype(np.float32)
        rec = (rng.standard_normal(((S, m, 3) if per_sample_rec else (m, 3))) * box).astype(np.float32)
        lig_r = RADII[rng.integers(0, len(RADII), n)]
        rec_r = np.concatenate([RADII, np.array([-1.0, -1.0], np.float32)])[rng.integers(0, len(RADII) + 2, m)]
        pairs = np.triu(rng.random((n, n)) < 0.5, 1).astype(np.uint8) if with_pairs else None
        bonds = np.stack([rng.permutation(n)[:2] for _ in range(T)]).astype(np.int64) if T else np.zeros((0, 2), np.int64)
        mask = rng.random((T, n)) < 0.4
        if T > 1:
            mask[-1] = False
            mask[-1, bonds[-1, 0]] = True
        upd0 = [rng.standard_normal((S, 3)).astype(np.float32), (0.3 * rng.standard_normal((S, 3))).astype(np.float32),
                (0.3 * rng.standard_normal((S, T))).astype(np.float32)]
        unit = forward(x, lig_r, rec, rec_r, pairs, bonds, mask, 1.0, (np.inf, np.inf, np.inf))
        need = (unit["norms"] / caps[None, :]).max(1)            # capped iff w * need > 1
        pos = np.sort(need[need > 0])
        if len(pos) == 0:
            w = 1.0
        elif S == 1 or pos[0] == pos[-1]:
            w = (2.0 if seed % 2 == 0 else 0.5) / pos[-1]
        else:
            w = 1.0 / np.sqrt(pos[0] * pos[-1])
        w = float(np.float32(w))
        ref = forward(x, lig_r, rec, rec_r, pairs, bonds, mask, w, caps, upd0)
        if margins_ok(ref, n):
            return dict(x=x, lig_r=lig_r, rec=rec, rec_r=rec_r, pairs=pairs, bonds=bonds, mask=mask, w=w, caps=caps, upd0=upd0, ref=ref,
                        need=need)
    raise AssertionError("no draw keeps the margins")


def rel_dev(got, want):
    """max |got - want| relative to the largest |want| (0 for empty arrays)."""
    want = np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), 1e-300))
