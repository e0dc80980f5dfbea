"""Float64 restatement of the SVGD particle-interaction term (the ddp_svgd_* definition of include/ddp_hip.h; reference
utils/sampling.py:197-242), in numpy, shared by tests/test_svgd_cpu.py, tests/test_gpu_svgd.py and tools/make_golden_svgd.py.
Independent of the package's two forms: the Kabsch rotation comes from numpy's SVD (the kernel takes Horn's quaternion route, the
PyTorch form a batched torch SVD), the axis-angle vector from the rotation MATRIX through the four quaternion candidates, as the
reference does it.  Also: the margins to the three discontinuities, and seeded pose sets."""
import math

import numpy as np

F64 = np.float64


def tau(pos, dih):
    """[N, T] signed dihedrals and their clamped cosines; pos [N, n, 3], dih [T, 4] = (c, a, b, d)."""
    pos = np.asarray(pos, F64)
    pc, pa, pb, pd = (pos[:, np.asarray(dih)[:, k]] for k in range(4))
    ab = pb - pa

    def normal_part(x):
        return x - (x * ab).sum(-1, keepdims=True) / (ab * ab).sum(-1, keepdims=True) * ab

    u, v = normal_part(pd - pa), normal_part(pc - pa)
    cos = (u * v).sum(-1) / (np.linalg.norm(u, axis=-1) * np.linalg.norm(v, axis=-1))
    clamped = np.clip(cos, -1 + 1e-5, 1 - 1e-5)
    return np.arccos(clamped) * np.sign((np.cross(u, v) * ab).sum(-1)), cos


def tor_diff(t):
    return np.fmod(t[:, None, :] - t[None, :, :] + 3 * math.pi, 2 * math.pi) - math.pi


def axis_angle(R):
    """(vector, q_abs sorted descending) of rotation matrices [..., 3, 3], the reference's matrix_to_axis_angle."""
    m = R.reshape(R.shape[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = np.moveaxis(m, -1, 0)
    q_abs = np.sqrt(np.maximum(np.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1), 0))
    cand = np.stack([np.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                     np.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
                     np.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
                     np.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * np.maximum(q_abs, 0.1)[..., None])
    best = q_abs.argmax(-1)
    q = np.take_along_axis(cand, best[..., None, None], -2)[..., 0, :]
    nrm = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    half = np.arctan2(nrm, q[..., :1])
    ang = 2 * half
    small = np.abs(ang) < 1e-6
    sha = np.where(small, 0.5 - ang * ang / 48, np.sin(half) / np.where(small, 1.0, ang))
    return q[..., 1:] / sha, -np.sort(-q_abs, -1)


def rigid(pos):
    """(tr_diff, rot_diff [N, N, 3], smallest gap between the largest q_abs and the runner-up over the pairs)."""
    pos = np.asarray(pos, F64)
    N = pos.shape[0]
    iu, ju = np.triu_indices(N, 1)
    cen = pos.mean(1)
    A, B = pos[iu] - cen[iu, None], pos[ju] - cen[ju, None]
    H = A.transpose(0, 2, 1) @ B
    U, _, Vt = np.linalg.svd(H)
    V, Ut = Vt.transpose(0, 2, 1), U.transpose(0, 2, 1)
    R = V @ Ut
    neg = np.linalg.det(R) < 0
    R[neg] = (V[neg] * np.array([1.0, 1.0, -1.0])) @ Ut[neg]
    vec, qs = axis_angle(R)
    tr, rot = np.zeros((N, N, 3)), np.zeros((N, N, 3))
    tr[iu, ju] = cen[ju] - cen[iu]
    rot[iu, ju] = vec
    return tr - tr.transpose(1, 0, 2), rot - rot.transpose(1, 0, 2), float((qs[:, 0] - qs[:, 1]).min())


def forward(pos, dih, scores, gdt, w_rep=1.0, w_rot=1.0, w_tor=1.0):
    """Steps 2-6: dict with tau, tr_diff, rot_diff, tor_diff, D, h, k, total = (tr, rot, tor or None) and the margins
    q_gap / wrap_gap (pi - max |tor_diff|) / cos_gap (1 - max |cos|).  scores = (tr [N, 3], rot [N, 3], tor [N, T] or None)."""
    pos = np.asarray(pos, F64)
    N = pos.shape[0]
    T = 0 if dih is None else len(dih)
    tr_d, rot_d, q_gap = rigid(pos)
    out = {"tr_diff": tr_d, "rot_diff": rot_d, "q_gap": q_gap, "wrap_gap": math.inf, "cos_gap": math.inf}
    D = (tr_d ** 2).sum(-1) + w_rot * (rot_d ** 2).sum(-1)
    if T:
        t, cos = tau(pos, dih)
        td = tor_diff(t)
        D = D + w_tor * (td ** 2).sum(-1)
        out.update(tau=t, tor_diff=td, wrap_gap=float(math.pi - np.abs(td).max()), cos_gap=float(1 - np.abs(cos).max()))
    med = np.sort(D, 1)[:, (N - 1) // 2]                       # torch.median: the lower middle value
    h = (w_rep * med / max(math.log(N), 1.0))[:, None]
    k = np.exp(-D / h)

    def total(score, diff, w, g):
        score = np.asarray(score, F64).reshape(N, -1)
        return g * (k @ score + ((2 / h * w * k)[:, :, None] * diff).sum(1)) / N

    out.update(D=D, h=h, k=k, total=(total(scores[0], tr_d, 1.0, gdt[0]), total(scores[1], rot_d, w_rot, gdt[1]),
                                     total(scores[2], out["tor_diff"], w_tor, gdt[2]) if T else None))
    return out


def update(base, total, weight, svgd_only):
    """Step 7 for one component: base = the SDE / ODE update a score + b z."""
    return weight * total + (0.0 if svgd_only else np.asarray(base, F64))


def margins_ok(r):
    """The three discontinuities are at a distance from the inputs: quaternion-candidate choice, +-pi wrap, cosine clamp."""
    return r["q_gap"] > 1e-3 and r["wrap_gap"] > 1e-3 and r["cos_gap"] > 1e-4


def rel_dev(got, want):
    """max |got - want| relative to the largest |want|."""
    want = np.asarray(want, F64)
    return float(np.abs(np.asarray(got, F64) - want).max() / np.abs(want).max())


def g2dt(sigma_ranges, t, dt):
    """[g_tr^2 dt, g_rot^2 dt, g_tor^2 dt] at diffusion time t (reference utils/sampling.py:129-130,145)."""
    s = sigma_ranges
    out = []
    for lo, hi, two in ((s.tr_sigma_min, s.tr_sigma_max, True), (s.rot_sigma_min, s.rot_sigma_max, False),
                        (s.tor_sigma_min, s.tor_sigma_max, True)):
        sigma = lo ** (1 - t) * hi ** t
        g = sigma * math.sqrt(2 * math.log(hi / lo)) if two else 2 * sigma * math.sqrt(math.log(hi / lo))
        out.append(g * g * dt)
    return out


def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def chain_poses(seed, N):
    """N poses of a 4-atom chain with one dihedral (0, 1, 2, 3): the smallest ligand the term is defined for.  float32 [N, 4, 3]."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-math.pi, math.pi, N)
    base = np.zeros((N, 4, 3))
    base[:, 0] = [1.0, 1.1, 0.0]
    base[:, 2] = [0.0, 0.0, 1.5]
    base[:, 3, 0], base[:, 3, 1], base[:, 3, 2] = 1.2 * np.cos(ang), 1.2 * np.sin(ang), 2.0
    pos = base @ random_rotations(rng, N).transpose(0, 2, 1) + rng.standard_normal((N, 1, 3)) * 2.0
    return pos.astype(np.float32), np.array([[0, 1, 2, 3]], np.int32)


def ligand_poses(seed, N):
    """N randomised poses of the 3dpf ligand (37 atoms, 5 rotatable bonds), as Sampler.randomize makes them (random torsions, uniform
    rotation, N(0, tr_sigma_max) translation), from the CPU sampler.  float32 [N, 37, 3]."""
    import torch
    from diffdock_pocket_amd import sampler as S
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    g = make_3dpf_complex(seed=0, flexible_sidechains=False, n_rec=8)
    smp = S.Sampler(None, g, N, torch.device("cpu"), S.SamplerConfig(flexible_sidechains=False), seed=seed)
    smp.randomize()
    return smp.lig_pos.numpy().astype(np.float32)
