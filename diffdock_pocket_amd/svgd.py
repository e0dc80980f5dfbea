"""The Stein variational (SVGD) particle-interaction term of the reverse-diffusion step: the one place where the N samples of a
complex interact (reference utils/sampling.py:197-242, utils/torsion.py:96-160, utils/geometry.py:100-206,246-281).

Two forms of the same arithmetic: the batched PyTorch one below (the CPU `Sampler.step`; the reference loops over the N (N - 1) / 2
pairs in Python with one 3x3 SVD each) and the three HIP launches of csrc/ddp_svgd.hip (`SvgdWorkspace`, the device step).  The
definition both follow is the ddp_svgd_* comment of include/ddp_hip.h.

Where the reference breaks, behaviour is defined: fewer than 3 samples raise (the median of a two-sample row is its zero diagonal:
h = 0, NaN), `torch.cross` runs over xyz (the reference's call without `dim` picks the first axis of size 3: wrong at N = 3 or
T = 3).  h_i = 0 - at least half of the poses coincide - is not special-cased.
"""
from __future__ import annotations

import math

import torch


def dihedrals(edge_index: torch.Tensor, edge_mask: torch.Tensor) -> torch.Tensor:
    """get_dihedrals (utils/torsion.py:96-113): int32 [T, 4] = (c, a, b, d) for every rotatable bond (a, b) in the order of the
    masked edge_index columns; c / d = the first neighbour of a / b in edge order that is not b / a."""
    ei = edge_index.cpu().long()
    nbrs: dict = {}
    for a, b in ei.t().tolist():
        nbrs.setdefault(a, []).append(b)
    out = []
    for (a, b), rot in zip(ei.t().tolist(), edge_mask.cpu().bool().tolist()):
        if not rot:
            continue
        c = next((x for x in nbrs.get(a, []) if x != b), None)
        d = next((x for x in nbrs.get(b, []) if x != a), None)
        if c is None or d is None:
            raise ValueError(f"rotatable bond ({a}, {b}) has an end without a second neighbour: no dihedral")
        out.append((c, a, b, d))
    return torch.tensor(out, dtype=torch.int32).reshape(-1, 4)


def torsion_angles(dih: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """tau [N, T] of poses pos [N, n, 3] (utils/torsion.py:120-135, cross product over xyz)."""
    d = dih.long()
    pc, pa, pb, pd = (pos[:, d[:, k]] for k in range(4))
    ab = pb - pa

    def normal_part(x):
        return x - (x * ab).sum(-1, keepdim=True) / (ab * ab).sum(-1, keepdim=True) * ab

    u, v = normal_part(pd - pa), normal_part(pc - pa)
    cos = (u * v).sum(-1) / (u.norm(dim=-1) * v.norm(dim=-1))
    cos = cos.clamp(-1 + 1e-5, 1 - 1e-5)
    sign = torch.sign((torch.cross(u, v, dim=-1) * ab).sum(-1))
    return torch.acos(cos) * sign


def torsion_diffs(tau: torch.Tensor) -> torch.Tensor:
    """tor_diff [N, N, T] = fmod(tau_i - tau_j + 3 pi, 2 pi) - pi (utils/torsion.py:138-145)."""
    return torch.fmod(tau.unsqueeze(1) - tau.unsqueeze(0) + 3 * math.pi, 2 * math.pi) - math.pi


def matrix_to_axis_angle(R: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] -> [..., 3] the way utils/geometry.py:100-206 does it: of the four quaternion candidates the one with the largest
    q_abs (its own component positive, the sign of w NOT standardised), angle = 2 atan2(|xyz|, w) - the vector can be longer than pi."""
    m = R.reshape(R.shape[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    q_abs = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1).clamp(min=0).sqrt()
    cand = torch.stack([torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs.unsqueeze(-1).clamp(min=0.1))
    best = q_abs.argmax(-1)
    q = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    nrm = q[..., 1:].norm(dim=-1, keepdim=True)
    half = torch.atan2(nrm, q[..., :1])
    ang = 2 * half
    small = ang.abs() < 1e-6
    sha = torch.where(small, 0.5 - ang * ang / 48, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    return q[..., 1:] / sha


def rigid_diffs(pos: torch.Tensor):
    """(tr_diff, rot_diff) [N, N, 3] of get_rigid_svgd (utils/torsion.py:148-160): the upper triangle from one batched SVD over the
    pairs, the lower one its negated mirror, the diagonal zero."""
    from .sampler import kabsch
    N = pos.shape[0]
    iu, ju = torch.triu_indices(N, N, offset=1, device=pos.device)
    R, _ = kabsch(pos[iu], pos[ju])
    cen = pos.mean(1)
    tr = pos.new_zeros(N, N, 3)
    rot = pos.new_zeros(N, N, 3)
    tr[iu, ju] = cen[ju] - cen[iu]
    rot[iu, ju] = matrix_to_axis_angle(R)
    return tr - tr.transpose(0, 1), rot - rot.transpose(0, 1)


def totals(pos, dih, tr_score, rot_score, tor_score, gdt, w_rep=1.0, w_rot=1.0, w_tor=1.0):
    """(total_tr [N, 3], total_rot [N, 3], total_tor [N, T] or None) of utils/sampling.py:198-225 for the pre-step poses pos [N, n, 3]
    and this step's scores; gdt = (g_tr^2 dt, g_rot^2 dt, g_tor^2 dt)."""
    N = pos.shape[0]
    if N < 3:
        raise ValueError("SVGD needs at least 3 samples: the median of a two-sample row is its zero diagonal")
    T = 0 if dih is None else int(dih.shape[0])
    tr_diff, rot_diff = rigid_diffs(pos)
    D = (tr_diff ** 2).sum(-1) + w_rot * (rot_diff ** 2).sum(-1)
    if T > 0:
        tor_diff = torsion_diffs(torsion_angles(dih, pos))
        D = D + w_tor * (tor_diff ** 2).sum(-1)
    h = w_rep * torch.median(D, dim=1, keepdim=True)[0] / max(math.log(N), 1.0)      # (torch.median: the LOWER middle value)
    k = torch.exp(-D / h)

    def total(score, diff, w, g):
        return g * (k @ score + (2 / h * w * k).unsqueeze(-1).mul(diff).sum(1)) / N

    return (total(tr_score.reshape(N, 3), tr_diff, 1.0, gdt[0]), total(rot_score.reshape(N, 3), rot_diff, w_rot, gdt[1]),
            total(tor_score.reshape(N, T), tor_diff, w_tor, gdt[2]) if T > 0 else None)


class SvgdWorkspace:
    """Device side: the dihedral table and the buffers the three passes of csrc/ddp_svgd.hip hand on, allocated once; `launch`
    enqueues the passes on the current stream (no host work besides the launches: capturable)."""

    def __init__(self, n, n_lig, dih, device, weight=1.0, w_rep=1.0, w_rot=1.0, w_tor=1.0, svgd_only=False):
        from . import _lib as L
        if n < 3:
            raise ValueError("SVGD needs at least 3 samples: the median of a two-sample row is its zero diagonal")
        if n_lig < 4:
            raise ValueError("SVGD needs a ligand of at least 4 atoms")
        T = 0 if dih is None else int(dih.shape[0])
        if T and (int(dih.min()) < 0 or int(dih.max()) >= n_lig):
            raise ValueError("dihedral atom index outside the ligand")
        self.n, self.n_lig, self.T = n, n_lig, T
        self.dih = dih.to(torch.int32).contiguous().to(device) if T else None
        self.tau = torch.zeros(n, T, dtype=torch.float64, device=device) if T else None
        self.tr_diff = torch.zeros(n, n, 3, device=device)
        self.rot_diff = torch.zeros(n, n, 3, device=device)
        self.tor_diff = torch.zeros(n, n, T, device=device) if T else None
        self.dist = torch.zeros(n, n, dtype=torch.float64, device=device)
        a = self.args = L.SvgdArgs()
        a.n, a.n_lig, a.n_tor = n, n_lig, T
        a.weight, a.w_rep, a.w_rot, a.w_tor, a.svgd_only = weight, w_rep, w_rot, w_tor, int(bool(svgd_only))
        a.dihedrals = self.dih.data_ptr() if T else None
        a.tau = self.tau.data_ptr() if T else None
        a.tr_diff, a.rot_diff, a.dist = self.tr_diff.data_ptr(), self.rot_diff.data_ptr(), self.dist.data_ptr()
        a.tor_diff = self.tor_diff.data_ptr() if T else None

    def launch(self, pos, scores, upd, gdt):
        """pos [n, n_lig, 3] (pre-step), scores / upd = (tr, rot, tor or None) fp32 contiguous device tensors, gdt = 3 floats in
        device memory.  upd is updated in place."""
        import ctypes as C
        from . import _lib as L
        lib = L.load()
        a = self.args
        for t, shape in ((pos, (self.n, self.n_lig, 3)), (scores[0], (self.n, 3)), (scores[1], (self.n, 3)), (upd[0], (self.n, 3)),
                         (upd[1], (self.n, 3))) + (((scores[2], (self.n, self.T)), (upd[2], (self.n, self.T))) if self.T else ()):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.numel() != math.prod(shape):
                raise ValueError(f"SvgdWorkspace.launch: fp32 contiguous device tensor of shape {shape} expected, got {tuple(t.shape)}")
        if gdt.dtype != torch.float32 or not gdt.is_cuda or gdt.numel() < 3 or not gdt.is_contiguous():
            raise ValueError("SvgdWorkspace.launch: gdt = 3 fp32 values in device memory")
        a.pos, a.gdt = pos.data_ptr(), gdt.data_ptr()
        for k in range(3):
            on = k < 2 or self.T > 0
            a.score[k] = scores[k].data_ptr() if on else None
            a.upd[k] = upd[k].data_ptr() if on else None
        st = torch._C._cuda_getCurrentRawStream(pos.device.index)
        L.check(lib.ddp_svgd_tau(C.byref(a), st), "ddp_svgd_tau")
        L.check(lib.ddp_svgd_pairs(C.byref(a), st), "ddp_svgd_pairs")
        L.check(lib.ddp_svgd_rows(C.byref(a), st), "ddp_svgd_rows")
