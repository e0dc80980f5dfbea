"""Relief of steric clashes of sampled poses, in pose space.  This project's own algorithm - NOT the reference's `--relax` (an OpenMM
force-field minimisation, which stays out of this tree).  It needs no force field, only what the package already defines: the van
der Waals table of assets/vdw_radii.json, the clash rule of ddp_pose_contacts (d < r_i + r_j - 2 overlap) and the sampler's own
degrees of freedom through ddp_pose_update / modify_conformer, so bond lengths, angles and rings cannot change.

Energy of one pose x against the pose x0 it started from, fp64 on the fp32 inputs (converted first), t_ij = r_i + r_j - 2 overlap,
pairs with t_ij <= 0 never count, receptor hydrogens (negative radius) are ignored:

    E = E_cross + E_self + E_rest
    E_cross = sum_{i lig, j rec} max(0, t_ij - d_ij)^2
    E_self  = the same sum over the ligand pairs of `self_pairs` (more than 3 bonds apart AND separated by a rotatable bond)
    E_rest  = k * mean_i |x_i - x0_i|^2

The search direction from the per-atom gradient dE/dx and the backtracking line search with its strict accept rule are those of
descent.py, which states them (the minimiser of minimize.py runs the same loop on another energy); the step constants are
RefineConfig's.  The pose update re-aligns the conformer after the torsions, so d_tor is not the exact derivative of the map that is
applied: the direction is a heuristic and the accept rule is what guarantees that the energy never rises.

What it does not do: no attraction or electrostatic term (it can only push atoms apart), no side-chain or receptor motion (the
receptor is static during the refinement; minimize_flex.py moves the flexible side chains with the ligand, in the physics score), no
hydrogens.

Device tensors go through descent.descend_hip with ddp_refine_energy (csrc/ddp_refine.hip) as the evaluation; CPU tensors through
descent.descend_torch with the PyTorch fp64 energy below."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .descent import DescentBuffers, descend_hip, descend_torch, direction_torch, ligand_torsions  # noqa: F401 (the last two: re-exported)
from .evaluation import OVERLAP_DISTANCE, PoseEvaluator
from .pose_args import check_anchor, check_poses
from .sampler import rotate_index_lists


@dataclass
class RefineConfig:
    """The constants of the line search.  Untuned choices, not fitted to anything."""
    iterations: int = 50          # fixed number of iterations
    restraint: float = 0.1        # k of E_rest
    step_init: float = 1.0        # first step size of every sample
    step_grow: float = 2.0        # factor after an accepted trial
    step_shrink: float = 0.5      # factor after a rejected trial
    step_max: float = 1024.0      # cap of the step size


@dataclass
class RefineResult:
    """Per-sample results of PoseRefiner.refine, in the order of the poses handed in, on their device."""
    lig_pos: torch.Tensor          # [S, n, 3] fp32 refined poses
    energy_before: torch.Tensor    # [S, 4] fp64: E_cross, E_self, E_rest, E
    energy_after: torch.Tensor     # [S, 4]
    clashes_before: torch.Tensor   # [S] int32, the clash count of PoseMetrics.clashes
    clashes_after: torch.Tensor    # [S] int32
    rmsd_moved: torch.Tensor       # [S] fp32 plain RMSD between the input and the refined pose
    accepted: torch.Tensor         # [S] int32 accepted trials

    def cpu(self) -> "RefineResult":
        return RefineResult(**{k: v.cpu() for k, v in self.__dict__.items()})


# ---------------------------------------------------------------------------------------------- host tables
def build_self_pairs(n: int, edge_index, mask_rotate) -> torch.Tensor:
    """uint8 [n, n], upper triangle: pair (i, j), i < j, counts iff its topological distance in the ligand bond graph is greater
    than 3 bonds (or there is no path) and some rotatable bond has mask_rotate[b][i] != mask_rotate[b][j], i.e. some torsion can
    change the distance."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    adj = np.zeros((n, n), dtype=bool)
    ok = (ei >= 0).all(0) & (ei < n).all(0) & (ei[0] != ei[1])
    adj[ei[0][ok], ei[1][ok]] = adj[ei[1][ok], ei[0][ok]] = True
    near = np.eye(n, dtype=bool)                     # within 0 bonds
    for _ in range(3):
        near = near | ((near.astype(np.int64) @ adj.astype(np.int64)) > 0)
    mask = np.asarray(mask_rotate, dtype=bool).reshape(-1, n)
    split = (mask[:, :, None] != mask[:, None, :]).any(0) if mask.shape[0] else np.zeros((n, n), dtype=bool)
    return torch.from_numpy(np.triu(~near & split, 1).astype(np.uint8))


# ---------------------------------------------------------------------------------------------- the PyTorch fp64 form
def _pair_terms(diff, t, ok):
    """diff [..., 3] fp64, t thresholds, ok mask (broadcast) -> (sum of max(0, t - d)^2 over the last two pair axes, dE/d(first atom)
    summed over the second)."""
    d = diff.pow(2).sum(-1).sqrt()
    pen = torch.where(ok, (t - d).clamp(min=0.0), torch.zeros_like(d))
    unit = torch.where((d > 0).unsqueeze(-1), diff / d.unsqueeze(-1), torch.zeros_like(diff))
    return pen.pow(2).sum((-1, -2)), ((-2.0 * pen).unsqueeze(-1) * unit).sum(-2)


def energy_torch(x, anchor, lig_r, rec, rec_r, self_pairs, overlap, restraint):
    """([S, 4] fp64 energies, [S, n, 3] fp64 gradient) of fp32 poses x against `anchor` - the definition of the module docstring."""
    S, n = x.shape[0], x.shape[1]
    x64, r64 = x.double(), lig_r.double()
    m = rec.shape[-2]
    e = torch.zeros(S, 4, dtype=torch.float64)
    g = torch.zeros(S, n, 3, dtype=torch.float64)
    t = r64[:, None] + rec_r.double()[None, :] - 2.0 * overlap
    ok = (rec_r[None, :] >= 0) & (t > 0)
    sp = None
    if self_pairs is not None and n > 1:
        sp = self_pairs.bool() | self_pairs.bool().T
        ts = r64[:, None] + r64[None, :] - 2.0 * overlap
        sp = sp & (ts > 0)
    chunk = max(1, (1 << 23) // max(1, n * max(m, n) * 3))
    for s0 in range(0, S, chunk):
        xs = x64[s0:s0 + chunk]
        if m > 0:
            r = (rec[None] if rec.dim() == 2 else rec[s0:s0 + chunk]).double()
            ec, gc = _pair_terms(xs[:, :, None, :] - r[:, None, :, :], t, ok)
            e[s0:s0 + chunk, 0] = ec
            g[s0:s0 + chunk] += gc
        if sp is not None:
            es, gs = _pair_terms(xs[:, :, None, :] - xs[:, None, :, :], ts, sp)
            e[s0:s0 + chunk, 1] = 0.5 * es               # every pair is met from both ends
            g[s0:s0 + chunk] += gs
    dx = x64 - anchor.double()
    e[:, 2] = restraint * dx.pow(2).sum(-1).mean(-1)
    g += (2.0 * restraint / n) * dx
    e[:, 3] = e[:, 0] + e[:, 1] + e[:, 2]
    return e, g


# ---------------------------------------------------------------------------------------------- refiner
class PoseRefiner:
    """Clash relief for the poses of one complex (see the module docstring).

    graph, device, receptor, overlap: as PoseEvaluator - receptor "graph" (the graph's atom nodes; each sample's own atom_pos when
    one is handed in: flexible runs) or (coords, elements), e.g. PoseEvaluator.full_receptor(pdb_text, graph.original_center).  Radii
    and the hydrogen convention are the evaluator's own tables; clash counts go through its contacts path."""

    def __init__(self, graph, device="cpu", receptor="graph", overlap: float = OVERLAP_DISTANCE, config: Optional[RefineConfig] = None):
        self.config = config or RefineConfig()
        if self.config.restraint < 0 or self.config.iterations < 0:
            raise ValueError("RefineConfig: restraint and iterations must not be negative")
        self.device = torch.device(device)
        self.overlap = float(overlap)
        self.evaluator = PoseEvaluator(graph, device, receptor=receptor, max_automorphisms=1, overlap=overlap)
        self.n, self.n_a = self.evaluator.n, self.evaluator.n_a
        self.bonds, self.mask_rotate = ligand_torsions(graph)
        self.T = int(self.bonds.shape[0])
        self.rot_idx = rotate_index_lists(self.mask_rotate)
        self.self_pairs = build_self_pairs(self.n, torch.as_tensor(graph["ligand", "ligand"].edge_index).numpy(), self.mask_rotate.numpy())
        self._ref_lig = torch.as_tensor(graph["ligand"].pos).float().reshape(-1, 3)
        if self.device.type != "cpu":
            from . import launch as LA
            self._bonds_i32 = LA.refine_bonds(self.bonds, self.n, self.device)      # checked on the host, uploaded once
            self._mask_u8 = self.mask_rotate.to(torch.uint8).contiguous().to(self.device)
            self._pairs_dev = self.self_pairs.contiguous().to(self.device)

    # ---- checks
    def _check(self, lig_pos, atom_pos):
        check_poses(self.n, self.n_a, self.device, lig_pos, atom_pos, "refiner")

    def _tables(self, lig_pos, atom_pos):
        apos = None if atom_pos is None else atom_pos.float().contiguous()
        return self.evaluator.contact_tables(lig_pos.is_cuda, apos)

    def clashes(self, lig_pos, atom_pos=None) -> torch.Tensor:
        """[S] int32 clash counts of the poses (PoseEvaluator.contacts: the count behind PoseMetrics.clashes)."""
        return self.evaluator.contacts(lig_pos, atom_pos)[:, 0].to(torch.int32)

    # ---- energy
    def energy(self, lig_pos, anchor=None, atom_pos=None):
        """([S, 4] fp64 = E_cross, E_self, E_rest, E; [S, n, 3] fp64 gradient) of the poses; anchor None: the poses themselves."""
        self._check(lig_pos, atom_pos)
        x = lig_pos.float().contiguous()
        a = x if anchor is None else anchor.float().contiguous()
        check_anchor(x, a)
        lig_r, rec, rec_r = self._tables(x, atom_pos)
        if not x.is_cuda:
            return energy_torch(x, a, lig_r, rec, rec_r, self.self_pairs, self.overlap, self.config.restraint)
        from . import launch as LA
        with torch.cuda.device(x.device):
            e = torch.empty(x.shape[0], 4, dtype=torch.float64, device=x.device)
            g = torch.empty(x.shape[0], self.n, 3, dtype=torch.float64, device=x.device)
            LA.refine_energy(LA.refine_args(x, a, lig_r, rec, rec_r, self._pairs_dev, self.overlap, self.config.restraint, e, g))
        return e, g

    # ---- refinement
    def refine(self, lig_pos, atom_pos=None, history: Optional[List[torch.Tensor]] = None) -> RefineResult:
        """Runs config.iterations iterations on lig_pos [S, n, 3] (flexible runs: atom_pos [S, n_a, 3], each sample's own static
        receptor) and returns a RefineResult on the poses' device.  The input tensor is not modified.  history: a list that receives
        the [S] total energies before the first and after every iteration (a debug hook; device tensors, no synchronisation)."""
        self._check(lig_pos, atom_pos)
        x0 = lig_pos.float().contiguous()
        lig_r, rec, rec_r = self._tables(x0, atom_pos)
        c = self.config
        S = x0.shape[0]
        step = torch.full((S,), float(c.step_init), dtype=torch.float64, device=x0.device)
        acc = torch.zeros(S, dtype=torch.int32, device=x0.device)
        if x0.is_cuda:
            from . import launch as LA
            with torch.cuda.device(x0.device):
                b = DescentBuffers(x0, self.T)
                common = dict(lig_radii=lig_r, rec=rec, rec_radii=rec_r, self_pairs=self._pairs_dev, overlap=self.overlap, restraint=c.restraint)
                cur = LA.refine_args(b.x, x0, bonds=self._bonds_i32, mask_rotate=self._mask_u8, step=step, accepted=acc, grow=c.step_grow,
                                     shrink=c.step_shrink, step_max=c.step_max, **b.refine_kwargs(), **common)
                tri = LA.refine_args(b.trial, x0, energy=b.et, grad=b.gt, **common)
                # (the loop evaluates b.x into b.e, b.g once and b.trial into b.et, b.gt from then on: both structs are built once)
                x, e0, e1 = descend_hip(lambda pos, e_out, g_out: LA.refine_energy(cur if pos is b.x else tri), cur, b, c.iterations,
                                        self._bonds_i32, self._mask_u8, history)
        else:
            x, _, acc, e0, e1 = descend_torch(lambda p: energy_torch(p, x0, lig_r, rec, rec_r, self.self_pairs, self.overlap, c.restraint),
                                              x0, step, acc, c.iterations, c, self.bonds, self.mask_rotate, self.rot_idx, self._ref_lig, history)
        moved = (x.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt().float()
        return RefineResult(x, e0, e1, self.clashes(x0, atom_pos), self.clashes(x, atom_pos), moved, acc)
