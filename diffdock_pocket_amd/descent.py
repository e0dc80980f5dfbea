"""The backtracking line search in pose space that the clash relief (refine.py) and the minimiser (minimize.py) share; each of them
brings its own energy and states the whole algorithm in its module docstring.

Search direction from the per-atom gradient g = dE/dx, each degree of freedom scaled by its unit-mass inertia (c the centroid, u^ the
unit axis x_u - x_v of bond (u, v), a_i = u^ x (x_i - x_v) over the atoms the bond rotates, u and v themselves left out: they lie on
the axis; a zero denominator gives 0):

    d_tr = -sum g_i / n      d_rot = -sum (x_i - c) x g_i / sum |x_i - c|^2      d_tor[b] = -sum g_i . a_i / sum |a_i|^2

One iteration, per sample with its own step size: trial = pose_update(x, step d_tr, step d_rot, step d_tor); the trial is taken iff
E(trial) < E(x) strictly in fp64 (a NaN energy is never accepted) and then step = min(grow step, step_max); otherwise x is kept bit
for bit and step = shrink step.  A fixed number of iterations, no convergence test, no host decision inside the loop.

Two forms of the loop: descend_torch, the fp64 PyTorch form on host tensors with sampler.modify_conformer as the pose update, and
descend_hip, launch by launch on device tensors (ddp_refine_direction, ddp_pose_update, the caller's evaluation, ddp_refine_accept:
energies, step sizes and accept counters stay in device memory, nothing synchronises).  The device side of the same pieces is
csrc/ddp_pose_descent.h."""
from __future__ import annotations

import torch

from .sampler import modify_conformer, modify_conformer_hip, torsion_tables


def ligand_torsions(graph):
    """(bonds [T, 2] int64 (u, v), mask_rotate [T, n] bool) of a complex graph: sampler.torsion_tables, the tables a Sampler hands to
    ddp_pose_update, checked against the ligand's size on the host."""
    n = int(graph["ligand"].pos.shape[0])
    bonds, mask = torsion_tables(graph)
    bonds, mask = torch.as_tensor(bonds).long().reshape(-1, 2), mask.reshape(-1, n)
    if mask.shape[0] != bonds.shape[0]:
        raise ValueError(f"mask_rotate has {mask.shape[0]} rows for {bonds.shape[0]} rotatable bonds")
    if bonds.numel() and (int(bonds.min()) < 0 or int(bonds.max()) >= n):
        raise ValueError(f"rotatable bond outside the ligand's {n} atoms")
    return bonds, mask


def direction_torch(x, g, bonds, mask_rotate):
    """fp64 (d_tr [S, 3], d_rot [S, 3], d_tor [S, T]) of the module docstring (not yet multiplied by the step)."""
    x = x.double()
    n = x.shape[1]
    zero = torch.zeros((), dtype=torch.float64)
    d_tr = -g.sum(1) / n
    p = x - x.mean(1, keepdim=True)
    den = p.pow(2).sum((1, 2))
    d_rot = torch.where(den[:, None] == 0, zero, -torch.cross(p, g, dim=-1).sum(1) / den[:, None])
    d_tor = torch.zeros(x.shape[0], bonds.shape[0], dtype=torch.float64)
    for b in range(bonds.shape[0]):
        u, v = int(bonds[b, 0]), int(bonds[b, 1])
        axis = x[:, u] - x[:, v]
        axis = axis / axis.norm(dim=-1, keepdim=True)
        mk = mask_rotate[b].bool().clone()
        mk[u] = mk[v] = False                              # the bond's own atoms lie on the axis: no lever, exactly
        a = torch.cross(axis[:, None, :].expand(-1, int(mk.sum()), -1), x[:, mk] - x[:, v:v + 1], dim=-1)
        num, dn = (g[:, mk] * a).sum((1, 2)), a.pow(2).sum((1, 2))
        d_tor[:, b] = torch.where(dn == 0, zero, -num / dn)
    return d_tr, d_rot, d_tor


def descend_torch(E, x0, step, acc, iterations, config, bonds, mask_rotate, rot_idx, ref_lig, history=None):
    """The CPU fp64 loop.  E(pos [S, n, 3] fp32) -> (e [S, 4] fp64 with the total in column 3, g [S, n, 3] fp64); start state x0, step
    [S] fp64, acc [S] int32 (none is modified); config: the step constants (RefineConfig or MinimizeConfig); bonds, mask_rotate: as
    ligand_torsions returns them, rot_idx: sampler.rotate_index_lists(mask_rotate); ref_lig [n, 3]: the graph's own ligand pose;
    history: a list that receives the [S] totals before the first and after every iteration.  Returns (x, step, acc, e0, e)."""
    c = config
    T = int(bonds.shape[0])
    x = x0.clone()
    e, g = E(x)
    e0 = e.clone()
    if history is not None:
        history.append(e[:, 3].clone())
    for _ in range(iterations if x.shape[0] else 0):
        d_tr, d_rot, d_tor = direction_torch(x, g, bonds, mask_rotate)
        # a sample without a finite energy can never accept (NaN compares false): the graph's own pose goes through the update in
        # its place with a zero move, so that its NaNs do not reach the batched SVD of the alignment
        fin = torch.isfinite(e[:, 3])
        tr, rot, tor = (torch.where(fin[:, None], step[:, None] * d, torch.zeros_like(d)).float() for d in (d_tr, d_rot, d_tor))
        trial = modify_conformer(torch.where(fin[:, None, None], x, ref_lig[None]), tr, rot, tor if T else None, bonds, rot_idx)
        et, gt = E(trial)
        take = et[:, 3] < e[:, 3]                      # strict, fp64; False for NaN
        x = torch.where(take[:, None, None], trial, x)
        g = torch.where(take[:, None, None], gt, g)
        e = torch.where(take[:, None], et, e)
        step = torch.where(take, (c.step_grow * step).clamp(max=c.step_max), c.step_shrink * step)
        acc = acc + take.to(torch.int32)
        if history is not None:
            history.append(e[:, 3].clone())
    return x, step, acc, e0, e


class DescentBuffers:
    """The device tensors of descend_hip for poses x0 [S, n, 3] with T rotatable bonds: the current pose x (a copy of x0) and the
    trial, their energies e, et [S, 4] and gradients g, gt [S, n, 3] fp64, the steps tr, rot [S, 3], tor [S, T] fp32."""

    def __init__(self, x0, T: int):
        dev, S, n = x0.device, x0.shape[0], x0.shape[1]
        f64 = dict(dtype=torch.float64, device=dev)
        self.x, self.trial = x0.clone(), torch.empty_like(x0)
        self.e, self.et = torch.empty(S, 4, **f64), torch.empty(S, 4, **f64)
        self.g, self.gt = torch.empty(S, n, 3, **f64), torch.empty(S, n, 3, **f64)
        self.tr, self.rot, self.tor = torch.empty(S, 3, device=dev), torch.empty(S, 3, device=dev), torch.empty(S, T, device=dev)

    def refine_kwargs(self):
        """The buffers under the names launch.refine_args takes them by."""
        return dict(energy=self.e, grad=self.g, tr=self.tr, rot=self.rot, tor=self.tor, trial=self.trial, trial_energy=self.et,
                    trial_grad=self.gt)


def descend_hip(evaluate, cur, buf: DescentBuffers, iterations, bonds_i32, mask_u8, history=None):
    """The device loop, launch by launch; it never synchronises.  evaluate(pos, e_out, g_out): energies [S, 4] and gradient of pos
    written into the two tensors; it is handed (buf.x, buf.e, buf.g) once and (buf.trial, buf.et, buf.gt) in every iteration.  cur:
    launch.refine_args of buf.x with buf.refine_kwargs(), the torsion tables, step, accepted and the step constants, for
    ddp_refine_direction and ddp_refine_accept (step and accepted are updated in place).  Returns (buf.x, e0, buf.e)."""
    from . import launch as LA
    T = buf.tor.shape[1]
    evaluate(buf.x, buf.e, buf.g)
    e0 = buf.e.clone()
    if history is not None:
        history.append(buf.e[:, 3].clone())
    for _ in range(iterations if buf.x.shape[0] else 0):
        LA.refine_direction(cur)
        # ddp_pose_update, the sampler's kernel: x -> trial (never in place: the accept kernel may have to keep x)
        modify_conformer_hip(buf.x, buf.tr, buf.rot, buf.tor if T else None, bonds_i32, mask_u8, out=buf.trial)
        evaluate(buf.trial, buf.et, buf.gt)
        LA.refine_accept(cur)
        if history is not None:
            history.append(buf.e[:, 3].clone())
    return buf.x, e0, buf.e
