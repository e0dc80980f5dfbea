"""NumPy float64 restatement of the side-chain part of the physics-score guidance term (diffdock_pocket_amd/score_guidance.py states
the definition, steps S1 - S4), independent of the package: nothing here imports it.

    g_y     = flexmin_ref.energy(x, y, x, y, ..., k = 0, k_sc = 0)["grad_y"]: dE/dy_a over the moving atoms, E = inter + intra + sc   (S1)
    d_sc[j] = -sum g_i . a_i / sum |a_i|^2 over the subcomponent of bond j = (u, v) without u and v, a_i = u^ x (y_i - y_v),
              u^ = (y_u - y_v) / |y_u - y_v|, a plain loop over the atoms; a zero denominator gives 0;  d32 = fp32(w d_sc)              (S2)
    f_sc    = min(1, max_sc / max_j |d32[j]|) in float64, a zero maximum: no constraint                                                (S3)
    increment = fp32(f_sc * fp64(d32));  upd = fp32(upd0 + increment)                                                                  (S4)

`bounds` - per element of upd_sc, composed in the style of score_guidance_ref.bounds / guidance_ref.bounds and derived, not fitted:
  * Both sides sum the same fp64 pair gradients in different orders: every component of g_y is off by at most bgy of
    flexmin_ref.bounds, 256 eps (P + 1) max(1, largest pair gradient).
  * num = sum over the k atoms of the bond's subcomponent of g_i . a_i: a dot product of three products, each a gradient component
    (error bgy) times a lever component (|a_i| <= L, the largest lever of the bond), is off by at most 3 L bgy per atom from its
    inputs, k 3 L bgy in all, plus 256 eps (k + 1) max(1, 3 L gmax) for its own summation and the fp64 roundings of the levers.
    den = sum |a_i|^2, k positive terms: off by at most 256 eps (k + 1) relative.  num / den inherits d_num / den + |num / den| d_den.
    Times w: the bound b_dir of the unrounded direction.
  * The cap factor is a continuous function of the maximum: where the cap can bind (max_sc / max <= 1 + 1e-6) its relative error is at
    most the relative error of the maximum, max_j b_dir[j] / max_j |d32[j]|; it multiplies the increment.
  * The three fp32 roundings of the definition (direction, increment, sum): 4 2^-24 (|upd0| + |increment|).
  bound = b_dir + |increment| rel_f + 4 2^-24 (|upd0| + |increment|)."""
import numpy as np

import flexmin_ref as F

EPS = 2.0 ** -53
U24 = 2.0 ** -24


def direction(y, gy, mov, edge, sub, mapping):
    """dict: the unweighted d [S, n_sc]; the margins bond_len [S, n_sc] and den [S, n_sc]; the magnitudes the bounds take: lever_max
    [S, n_sc] and count [n_sc] (moving atoms of the bond's subcomponent off its axis).  A plain loop over samples, bonds and atoms."""
    y = np.asarray(y, np.float64)
    S = y.shape[0]
    slot = {int(a): r for r, a in enumerate(np.asarray(mov).tolist())}
    edge, mapping = np.asarray(edge, np.int64).reshape(-1, 2), np.asarray(mapping, np.int64).reshape(-1, 2)
    n_sc = edge.shape[0]
    out = dict(d=np.zeros((S, n_sc)), bond_len=np.zeros((S, n_sc)), den=np.zeros((S, n_sc)), lever_max=np.zeros((S, n_sc)),
               count=np.zeros(n_sc))
    for j in range(n_sc):
        u, v = int(edge[j, 0]), int(edge[j, 1])
        atoms = [int(a) for a in np.asarray(sub)[int(mapping[j, 0]):int(mapping[j, 1])].tolist() if a != u and a != v and int(a) in slot]
        out["count"][j] = len(atoms)
        for s in range(S):
            axis = y[s, u] - y[s, v]
            ln = float(np.sqrt(axis @ axis))
            out["bond_len"][s, j] = ln
            num = den = 0.0
            for a in atoms:
                lever = np.cross(axis / ln, y[s, a] - y[s, v])
                num += float(gy[s, slot[a]] @ lever)
                den += float(lever @ lever)
                out["lever_max"][s, j] = max(out["lever_max"][s, j], float(np.sqrt(lever @ lever)))
            out["den"][s, j] = den
            out["d"][s, j] = 0.0 if den == 0.0 else -num / den
    return out


def cap_factor(d32, max_sc):
    """(f_sc [S] float64, mx [S]) from the fp32 direction d32 [S, n_sc]."""
    S = d32.shape[0]
    mx = np.abs(d32.astype(np.float64)).max(1) if d32.shape[1] else np.zeros(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(mx > 0, np.minimum(1.0, max_sc / mx), 1.0)
    return f, mx


def forward(c, w, max_sc, upd0=None, consts=None, kink=True):
    """The whole definition for a case dict (the keys of flexmin_ref.random_case: x, y, lig_r, lig_f, rec_r, rec_f, pairs, mov, edge,
    sub, mapping, sc_pairs) and the fp32 weight w.  dict: fm (flexmin_ref.energy at k = k_sc = 0, anchors = the state), dr
    (direction), d32, f, mx, inc (fp32), upd (fp32, when upd0 [S, n_sc] is given), capped [S] bool, cutoff_gap, kink_gap
    (flexmin_ref.kink_distance; kink=False: not computed, infinity)."""
    w = float(np.float32(w))
    fm = F.energy(c["x"], c["y"], c["x"], c["y"], c["lig_r"], c["lig_f"], c["rec_r"], c["rec_f"], c["pairs"], c["mov"], c["sc_pairs"], 0.0, 0.0,
                  consts)
    dr = direction(c["y"], fm["grad_y"], c["mov"], c["edge"], c["sub"], c["mapping"])
    d32 = (w * dr["d"]).astype(np.float32)
    f, mx = cap_factor(d32, max_sc)
    inc = (f[:, None] * d32.astype(np.float64)).astype(np.float32)
    out = dict(fm=fm, dr=dr, d32=d32, f=f, mx=mx, inc=inc, capped=f < 1.0, w=w, max_sc=float(max_sc), cutoff_gap=fm["cutoff_gap"],
               kink_gap=F.kink_distance(c, consts) if kink else np.inf)
    if upd0 is not None:
        out["upd"] = (np.asarray(upd0, np.float32) + inc).astype(np.float32)
    return out


def margins_ok(ref, kink_gap=1e-6):
    """No pair within 1e-6 A of the cutoff, none inside the cutoff within kink_gap of a ramp end (the gradient jumps there), every
    side-chain bond longer than 1e-3 A and, where it turns an atom, a lever sum above 1e-6."""
    dr = ref["dr"]
    turning = dr["count"] > 0
    return bool(ref["cutoff_gap"] >= 1e-6) and bool(ref["kink_gap"] >= kink_gap) and bool((dr["bond_len"] > 1e-3).all()) and \
        bool((dr["den"][:, turning] > 1e-6).all())


def bounds(ref, upd0=None):
    """[S, n_sc]: the bound of the module docstring per element of upd_sc (or of the increment when upd0 is None)."""
    fm, dr, w = ref["fm"], ref["dr"], ref["w"]
    bgy = F.bounds(fm)[2]
    gmax = np.abs(fm["grad_y"]).max((1, 2)) if fm["grad_y"].size else np.zeros(bgy.shape)
    k, L = dr["count"][None, :], dr["lever_max"]
    ownk = 256.0 * EPS * (k + 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        b_dir = np.where(dr["den"] > 0, w * ((k * 3.0 * L * bgy[:, None] + ownk * np.maximum(1.0, 3.0 * L * gmax[:, None])) / dr["den"]
                                             + np.abs(dr["d"]) * ownk), 0.0)
        mx = ref["mx"]
        worst = b_dir.max(1) if b_dir.shape[1] else np.zeros_like(mx)
        rel = np.where(mx > 0, worst / mx, 0.0)
        binding = np.where(mx > 0, ref["max_sc"] / mx <= 1.0 + 1e-6, False)
    relf = np.where(binding, rel, 0.0)
    inc = np.abs(ref["inc"].astype(np.float64))
    u0 = np.abs(np.asarray(upd0, np.float64)) if upd0 is not None else 0.0
    return b_dir + inc * relf[:, None] + 4.0 * U24 * (u0 + inc)


def random_case(S, n, m, n_mov, n_sc, seed, max_sc=0.5, **kw):
    """flexmin_ref.random_case(..., kink_gap=1e-6 unless given) with what the term adds: the weight w, chosen from the unweighted
    direction so that, with S > 1, the sample that needs the side-chain cap most is capped and the one that needs it least is not
    (S = 1 or no spread: capped for even seeds, uncapped for odd ones; w stays inside [2^-10, 2^10]); upd0 [S, n_sc], a random preload; a few random ligand torsions
    (bonds [T, 2], mask [T, n], T = min(3, n - 1)) for the ligand part of the kernel; ref = forward."""
    kw.setdefault("kink_gap", 1e-6)
    c = F.random_case(S, n, m, n_mov, n_sc, seed, **kw)
    rng = np.random.default_rng(seed + 5)
    T = min(3, n - 1)
    c["bonds"] = np.stack([rng.permutation(n)[:2] for _ in range(T)]).astype(np.int64) if T else np.zeros((0, 2), np.int64)
    c["mask"] = rng.random((T, n)) < 0.4
    c["upd0"] = (0.3 * rng.standard_normal((S, n_sc))).astype(np.float32)
    c["upd0_lig"] = [rng.standard_normal((S, 3)).astype(np.float32), (0.3 * rng.standard_normal((S, 3))).astype(np.float32),
                     (0.3 * rng.standard_normal((S, T))).astype(np.float32)]
    unit = forward(c, 1.0, np.inf, kink=False)
    need = unit["mx"] / max_sc                                    # capped iff w * need > 1
    pos = np.sort(need[need > 0])
    if len(pos) == 0:
        w = 1.0
    elif S == 1 or pos[0] == pos[-1]:
        w = (2.0 if seed % 2 == 0 else 0.5) / pos[-1]
    else:
        w = 1.0 / np.sqrt(pos[0] * pos[-1])
    w = min(max(w, 2.0 ** -10), 2.0 ** 10)                        # (a direction that is numerically nothing is not blown up to the cap)
    c["w"], c["max_sc"], c["need"] = float(np.float32(w)), float(max_sc), need
    c["sg"] = forward(c, c["w"], max_sc, c["upd0"])
    return c
