"""An independent NumPy fp64 restatement of the joint energy of diffdock_pocket_amd/minimize_flex.py and both its gradients, for the
tests of the PyTorch form and of csrc/ddp_minimize_flex.hip.  The pairs are listed by plain loops; the pair terms are vinardo_ref's.  It imports
nothing from the package and accepts fp64 coordinates (the finite-difference tests move them by less than an fp32 ulp).

    E(x, y) = inter(x, y) + intra(x) + sc(y) + k mean_i |x_i - x0_i|^2 + k_sc mean_{a in mov} |y_a - y0_a|^2
    sc(y): the weighted pair terms over the receptor pairs {a, b} listed in sc_pairs [n_mov, m] (row r: the partners of mov[r]), every
    unordered pair once; both atoms typed.  A table that lists a pair of two moving atoms in one row only is rejected.
    d/dx_i as vinardo_ref + the restraint;  d/dy_a, a in mov: d inter/dy_a + d sc/dy_a + (2 k_sc / n_mov)(y_a - y0_a)."""
import numpy as np

import vinardo_ref as V


def sc_pair_list(mov, sc_pairs, rec_r):
    """The unordered typed pairs (a, b) of the table, a in mov: every pair once."""
    mov = [int(a) for a in mov]
    slot = {a: r for r, a in enumerate(mov)}
    out = []
    for r, a in enumerate(mov):
        for b in np.nonzero(np.asarray(sc_pairs)[r])[0].tolist():
            if b == a:
                continue
            if b in slot:
                assert sc_pairs[slot[b]][a], f"pair ({a}, {b}) of two moving atoms is in one row only"
                if b < a:
                    continue                      # met from b's row
            if rec_r[a] >= 0 and rec_r[b] >= 0:
                out.append((a, b))
    return out


def energy(x, y, x0, y0, lig_r, lig_f, rec_r, rec_f, pairs, mov, sc_pairs, k=0.0, k_sc=0.0, c=None):
    """x, x0 [S, n, 3], y, y0 [S, m, 3] (any float type: converted to fp64 first).  Returns a dict:
      energy [S, 6] = inter, intra, sc, ligand restraint term, side-chain restraint term, E
      grad_x [S, n, 3], grad_y [S, n_mov, 3]
      n_pairs [S, 6], max_term [S, 6]: the summands behind every energy entry and the largest |summand| (pairs inside the cutoff and
        weighted pair terms for inter, intra and sc; 3 n and 3 n_mov squares for the restraints; E: the sums of the others)
      n_pairs_gx [S], max_gx [S], n_pairs_gy [S], max_gy [S]: summands of a gradient component (pairs inside the cutoff that touch
        the molecule, + 1 for the restraint) and the largest of them
      cutoff_gap: min over all pairs met, cross, self or sc, of |d - cutoff|.
    c: a vinardo_ref.Constants (None: the defaults)."""
    c = c or V.DEFAULT
    x, y, x0, y0 = (np.asarray(a, dtype=np.float64) for a in (x, y, x0, y0))
    S, n = x.shape[:2]
    mov = np.asarray(mov, dtype=np.int64).reshape(-1)
    n_mov = len(mov)
    rec_r64 = np.asarray(rec_r, dtype=np.float64)
    rec_f64 = np.asarray(rec_f).astype(np.int64)
    ref = V.score(x, lig_r, lig_f, y, rec_r, rec_f, pairs, 1.0, c)
    out = {"energy": np.zeros((S, 6)), "grad_x": ref["grad"].copy(), "grad_y": np.zeros((S, n_mov, 3)), "n_pairs": np.zeros((S, 6)),
           "max_term": np.zeros((S, 6)), "n_pairs_gx": ref["n_pairs_grad"] + 1.0, "max_gx": ref["max_grad"].copy(),
           "n_pairs_gy": np.zeros(S), "max_gy": np.zeros(S), "cutoff_gap": ref["cutoff_gap"]}
    plist = sc_pair_list(mov, sc_pairs, rec_r64)
    slot = {int(a): r for r, a in enumerate(mov)}
    lig_r64, lig_f64 = np.asarray(lig_r, dtype=np.float64), np.asarray(lig_f).astype(np.int64)
    for s in range(S):
        e = out["energy"][s]
        e[0], e[1] = ref["energy"][s, 4], ref["energy"][s, 5]
        out["n_pairs"][s, :2] = ref["n_pairs"][s, 4:6]
        out["max_term"][s, :2] = ref["max_term"][s, 4:6]
        gy = out["grad_y"][s]
        n_gy, max_gy = 0, 0.0
        # d inter / dy_a: the typed pairs (moving atom a, ligand atom i), the moving atom first
        ia = np.array([(r, a, i) for r, a in enumerate(mov.tolist()) if rec_r64[a] >= 0 for i in range(n) if lig_r64[i] >= 0],
                      dtype=np.int64).reshape(-1, 3)
        if len(ia):
            inside, _, pg, _ = V.pair_terms(y[s, ia[:, 1]] - x[s, ia[:, 2]], rec_r64[ia[:, 1]] + lig_r64[ia[:, 2]], rec_f64[ia[:, 1]], lig_f64[ia[:, 2]], c)
            np.add.at(gy, ia[:, 0], pg)
            n_gy += int(inside.sum())
            max_gy = max(max_gy, float(np.sqrt((pg ** 2).sum(-1)).max()))
        # sc: every unordered pair once; the second atom gets the opposite gradient if it moves
        t_sum, n_sc_pairs, max_w = np.zeros(4), 0, 0.0
        if plist:
            pa, pb = np.array(plist, dtype=np.int64).T
            inside, t, pg, d = V.pair_terms(y[s, pa] - y[s, pb], rec_r64[pa] + rec_r64[pb], rec_f64[pa], rec_f64[pb], c)
            if np.isfinite(d).any():
                out["cutoff_gap"] = min(out["cutoff_gap"], float(np.nanmin(np.abs(d - c.cutoff))))
            t_sum, n_sc_pairs, max_w = t.sum(0), int(inside.sum()), float(np.abs(t @ V.weights(c)).max())
            np.add.at(gy, np.array([slot[int(a)] for a in pa]), pg)
            second = np.array([slot.get(int(b), -1) for b in pb])
            np.add.at(gy, second[second >= 0], -pg[second >= 0])
            n_gy += n_sc_pairs
            max_gy = max(max_gy, float(np.sqrt((pg ** 2).sum(-1)).max()))
        e[2] = V.weights(c) @ t_sum
        out["n_pairs"][s, 2], out["max_term"][s, 2] = n_sc_pairs, max_w
        # restraints
        dx = x[s] - x0[s]
        tx = k * dx ** 2 / n
        e[3] = tx.sum()
        out["grad_x"][s] += (2.0 * k / n) * dx
        out["n_pairs"][s, 3], out["max_term"][s, 3] = 3 * n, tx.max()
        out["max_gx"][s] = max(out["max_gx"][s], (2.0 * k / n) * np.abs(dx).max())
        if n_mov:
            dy = y[s, mov] - y0[s, mov]
            ty = k_sc * dy ** 2 / n_mov
            e[4] = ty.sum()
            gy += (2.0 * k_sc / n_mov) * dy
            out["n_pairs"][s, 4], out["max_term"][s, 4] = 3 * n_mov, ty.max()
            max_gy = max(max_gy, (2.0 * k_sc / n_mov) * np.abs(dy).max())
        e[5] = e[0] + e[1] + e[2] + e[3] + e[4]
        out["n_pairs"][s, 5] = out["n_pairs"][s, :5].sum()
        out["max_term"][s, 5] = out["max_term"][s, :5].max()
        out["n_pairs_gy"][s], out["max_gy"][s] = n_gy + 1.0, max_gy
    return out


def bounds(ref):
    """The bound form of vinardo_ref.bounds, 256 eps (P + 1) max(1, largest |summand|), per energy entry [S, 6] and per component of
    the two gradients ([S], [S]).  E is the sum of its five parts: its bound is the sum of theirs."""
    be = 256.0 * V.EPS * (ref["n_pairs"] + 1.0) * np.maximum(1.0, ref["max_term"])
    be[:, 5] = be[:, :5].sum(1)
    bgx = 256.0 * V.EPS * (ref["n_pairs_gx"] + 1.0) * np.maximum(1.0, ref["max_gx"])
    bgy = 256.0 * V.EPS * (ref["n_pairs_gy"] + 1.0) * np.maximum(1.0, ref["max_gy"])
    return be, bgx, bgy


def apply_sidechains(y, edge, sub, mapping, angles):
    """fp64 restatement of the side-chain map: bond j turns y[sub[mapping[j, 0]:mapping[j, 1]]] by angles[j] about y_u - y_v through y_v
    (Rodrigues), bonds in list order.  y [m, 3]."""
    y = np.array(y, dtype=np.float64)
    for j in range(len(edge)):
        u, v = int(edge[j][0]), int(edge[j][1])
        ax = y[u] - y[v]
        ax = ax / np.linalg.norm(ax)
        idx = np.asarray(sub[int(mapping[j][0]):int(mapping[j][1])], dtype=np.int64)
        p = y[idx] - y[v]
        c, s = np.cos(angles[j]), np.sin(angles[j])
        y[idx] = p * c + np.cross(ax[None], p) * s + ax[None] * (p @ ax)[:, None] * (1.0 - c) + y[v]
    return y


def random_case(S, n, m, n_mov, n_sc, seed, with_pairs=True, untyped_moving=False, moving_at=None, kink_gap=0.0, c=None):
    """vinardo_ref.random_case with per-sample receptors, plus random side-chain tables: mov (sorted; `moving_at`: these receptor indices
    are among them; untyped_moving: the first moving atom is untyped, otherwise every moving atom is typed), n_sc bonds (u, v: two
    receptor atoms outside the bond's subcomponent, which is a random non-empty subset of mov), sc_pairs [n_mov, m] (random, symmetric
    among the moving atoms, never an atom with itself).  Start state x0, y0: the state plus noise (y0 differs on the moving atoms only).
    Redrawn until no pair, cross, self or sc, lies within 1e-6 A of the cutoff and, with kink_gap > 0, no pair inside the cutoff has
    its surface distance s within kink_gap of a kink of the ramps (0, 2.5, -0.6).  Returns a dict of fp32 / integer NumPy arrays and
    `ref`, the restatement's result with k = 0.7, k_sc = 0.3 (the keys `k`, `k_sc`).  c: the constants of the reference, the cutoff and
    the kinks (None: the defaults, to which the numbers above belong)."""
    assert n_mov <= m and (n_sc == 0 or (n_mov >= 1 and m >= 3))
    for t in range(256):
        sd = seed + 7919 * t
        x, lig_r, lig_f, y, rec_r, rec_f, pairs, _ = V.random_case(S, n, m, sd, True, with_pairs, c)
        rng = np.random.default_rng(sd + 1)
        fixed = sorted(set(moving_at or []))
        rest = [a for a in rng.permutation(m).tolist() if a not in fixed][:n_mov - len(fixed)]
        mov = np.array(sorted(fixed + rest), dtype=np.int64)
        rec_r = rec_r.copy()
        table = np.array(list(V.RADII.values()), dtype=np.float32)
        rec_r[mov] = table[rng.integers(0, len(table), n_mov)]
        if untyped_moving and n_mov:
            rec_r[mov[0]] = -1.0
        edge, sub, mapping = [], [], []
        for j in range(n_sc):
            size = int(rng.integers(1, n_mov + 1))
            if m - size < 2:
                size = m - 2
            comp = sorted(rng.permutation(n_mov)[:size].tolist())
            others = [a for a in rng.permutation(m).tolist() if a not in set(mov[comp].tolist())]
            edge.append([others[0], others[1]])
            mapping.append([len(sub), len(sub) + size])
            sub += mov[comp].tolist()
        sc_pairs = (rng.random((n_mov, m)) < 0.6).astype(np.uint8)
        for r, a in enumerate(mov.tolist()):
            sc_pairs[r, a] = 0
            for r2, b in enumerate(mov.tolist()):
                if r2 > r:
                    sc_pairs[r2, a] = sc_pairs[r, b]
        x0 = (x + 0.25 * rng.standard_normal(x.shape)).astype(np.float32)
        y0 = y.copy()
        y0[:, mov] += (0.25 * rng.standard_normal((S, n_mov, 3))).astype(np.float32)
        case = {"x": x, "y": y, "x0": x0, "y0": y0, "lig_r": lig_r, "lig_f": lig_f, "rec_r": rec_r, "rec_f": rec_f, "pairs": pairs, "mov": mov,
                "edge": np.array(edge, dtype=np.int64).reshape(-1, 2), "sub": np.array(sub, dtype=np.int64),
                "mapping": np.array(mapping, dtype=np.int64).reshape(-1, 2), "sc_pairs": sc_pairs, "k": 0.7, "k_sc": 0.3}
        ref = energy(x, y, x0, y0, lig_r, lig_f, rec_r, rec_f, pairs, mov, sc_pairs, 0.7, 0.3, c)
        if ref["cutoff_gap"] < 1e-6:
            continue
        if kink_gap > 0 and kink_distance(case, c) < kink_gap:
            continue
        case["ref"] = ref
        return case
    raise AssertionError("no draw clear of the cutoff and the kinks")


def kink_distance(case, c=None):
    """min over all typed pairs of the case inside cutoff + 0.1 of the distance of s = d - R_a - R_b to a kink of the ramps and of the
    repulsion (0, 2.5, -0.6) and of d to the cutoff: how far a finite-difference step may reach.  c: a vinardo_ref.Constants (None: the
    defaults, to which the numbers above belong): the kinks are 0 and the four ends of its ramps."""
    c = c or V.DEFAULT
    kinks = (0.0, c.hydrophobic_good, c.hydrophobic_bad, c.hbond_good, c.hbond_bad)
    x, y = case["x"].astype(np.float64), case["y"].astype(np.float64)
    lig_r, rec_r = case["lig_r"].astype(np.float64), case["rec_r"].astype(np.float64)
    worst = np.inf

    def visit(d, rsum):
        nonlocal worst
        if d < c.cutoff + 0.1:
            s = d - rsum
            worst = min(worst, abs(d - c.cutoff), *(abs(s - k) for k in kinks))

    for s in range(x.shape[0]):
        for i in np.nonzero(lig_r >= 0)[0]:
            for j in np.nonzero(rec_r >= 0)[0]:
                visit(np.linalg.norm(x[s, i] - y[s, j]), lig_r[i] + rec_r[j])
        if case["pairs"] is not None:
            for i, j in zip(*np.nonzero(np.triu(case["pairs"], 1))):
                if lig_r[i] >= 0 and lig_r[j] >= 0:
                    visit(np.linalg.norm(x[s, i] - x[s, j]), lig_r[i] + lig_r[j])
        for a, b in sc_pair_list(case["mov"], case["sc_pairs"], rec_r):
            visit(np.linalg.norm(y[s, a] - y[s, b]), rec_r[a] + rec_r[b])
    return worst
