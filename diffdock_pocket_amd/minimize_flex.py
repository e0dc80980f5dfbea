"""Local minimisation of a sampled pose TOGETHER with the flexible side chains of its receptor, in the Vinardo-form score of
scoring.py: the joint form of minimize.py.  minimize.py moves the ligand against each sample's fixed side chains; here the chi angles
of the flexible residues (flexResidues of the graph, the degrees of freedom the sampler itself moves through
sampler.apply_sidechain_torsions) descend with the ligand's translation, rotation and torsions, in one line search.

State per pose: the ligand x [n, 3] and the receptor atoms y [m, 3] (the graph's atom nodes, each sample's own atom_pos), fp32.  Mv,
the moving set, is the sorted unique entries of flexResidues.subcomponents; every other receptor atom never changes.  Energy against
the start (x0, y0), fp64 on the fp32 inputs (converted first):

    E(x, y) = inter(x, y) + intra(x) + sc(y) + k * mean_i |x_i - x0_i|^2 + k_sc * mean_{a in Mv} |y_a - y0_a|^2

inter and intra are scoring.py's, exactly as in minimize.py (the same ScoreConfig, typing, cutoff and NaN rule).  sc(y) is the same
weighted sum of the four pair terms (same weights, radii, flags, cutoff) over the receptor pairs {a, b} with at least one atom in Mv,
every unordered pair once, that are more than 3 bonds apart in the receptor bond graph (scoring.distance_bonds on the graph's own atom
positions) AND separated by a side-chain torsion (some bond's subcomponent contains exactly one of the two): the rule of
refine.build_self_pairs for the ligand, stated per moving atom by `build_sc_pairs` (two static atoms are never a pair).  Untyped
atoms take part in nothing.  Defaults k = k_sc = 0.
Gradient: with respect to x as in minimize.py; with respect to y_a, a in Mv: d inter/dy_a + d sc/dy_a + (2 k_sc / |Mv|)(y_a - y0_a).

Direction: the ligand's is descent.direction_torch, unchanged.  Side-chain bond j = (u, v) with subcomponent C_j gets the same inertia
scaling as a ligand torsion: d_sc[j] = -sum g_i . a_i / sum |a_i|^2 over i in C_j without u and v, a_i = u^ x (y_i - y_v),
u^ = (y_u - y_v) / |y_u - y_v|; a zero denominator gives 0.  There is no re-alignment on the receptor side, so at the current pose this
IS the first derivative of E with respect to angle j (divided by sum |a_i|^2), whatever the order the bonds are applied in.

One iteration, one step size per pose for both molecules: x' = modify_conformer(x, step d_tr, step d_rot, step d_tor),
y' = apply_sidechain_torsions(y, step d_sc) (bonds in list order, as the sampler applies them; the fp32 arguments are rounded from
fp64); the trial is taken iff E(x', y') < E(x, y) strictly in fp64 (NaN is never accepted) and then step = min(grow step, step_max);
otherwise x and y are kept bit for bit and step = shrink step.  A fixed number of iterations, no host decision in the loop: the loop of
descent.descend_torch with a second molecule in the state (descend_flex_torch below).

What this is and is not.  In form it is Vina's treatment of flexible residues: the flexible atoms see the rigid receptor and each other
through the same pair terms as the ligand does.  It is this package's own algorithm and NOT the reference's `--relax` (an OpenMM
force-field minimisation).  No backbone motion, no hydrogens, no rotamer library, no global search: a local descent from the sampled
rotamers.  The constants are Vinardo's published ones, not fitted here, and the score is still not validated against smina or Vina.

Forms: CPU tensors run descend_flex_torch on the fp64 energy below; this form is the definition.  Device tensors run
csrc/ddp_minimize_flex.hip (ddp_pose_minimize_flex): one workgroup per pose holds both molecules' state in LDS and runs all iterations
in ONE launch.  Above the kernel's limits (DDP_MINIMIZE_FLEX_MAX_MOVING moving atoms, DDP_MINIMIZE_FLEX_MAX_BONDS side-chain bonds,
DDP_MINIMIZE_FLEX_MAX_STATE_BYTES of per-atom LDS state, and the ligand limits of ddp_pose_minimize) the class warns once, naming the
limit, and runs the CPU form on host copies: the same algorithm.  The device form follows the CPU form up to rounding, as
minimize.py's does."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .descent import direction_torch
from .minimize import MinimizeConfig, PoseMinimizer, _warn_once
from .sampler import apply_sidechain_torsions, modify_conformer
from .scoring import ATOMIC_NUMS, PoseScores, ScoreConfig, _pair_sums, _weighted, distance_bonds, score_torch


@dataclass
class FlexMinimizeResult:
    """Per-sample results of FlexPoseMinimizer.minimize, in the order of the poses handed in, on their device."""
    lig_pos: torch.Tensor                # [S, n, 3] fp32 minimised poses
    atom_pos: torch.Tensor               # [S, m, 3] fp32 receptor atoms with the minimised side chains
    energy_before: torch.Tensor          # [S, 6] fp64: inter, intra, sc, ligand restraint term, side-chain restraint term, E
    energy_after: torch.Tensor           # [S, 6]
    scores_before: PoseScores            # PoseScorer.score of the poses handed in against the side chains handed in
    scores_after: PoseScores             # PoseScorer.score of lig_pos against atom_pos
    rmsd_moved: torch.Tensor             # [S] fp32 plain RMSD between the input and the minimised ligand pose
    sidechain_rmsd_moved: torch.Tensor   # [S] fp32 the same over the moving atoms Mv
    accepted: torch.Tensor               # [S] int32 accepted trials

    def cpu(self) -> "FlexMinimizeResult":
        return FlexMinimizeResult(**{k: v.cpu() for k, v in self.__dict__.items()})

    def index(self, order) -> "FlexMinimizeResult":
        return FlexMinimizeResult(**{k: (v.index(order) if isinstance(v, PoseScores) else v[order.to(v.device)])
                                     for k, v in self.__dict__.items()})


# ---------------------------------------------------------------------------------------------- host tables
@dataclass
class SidechainTables:
    """The side-chain degrees of freedom of one complex, host tensors: mov [n_mov] int64 (Mv, sorted unique), edge_idx [n_sc, 2] (u, v),
    sub / mapping (bond j turns sub[mapping[j, 0]:mapping[j, 1]]), pairs uint8 [n_mov, m] (build_sc_pairs)."""
    mov: torch.Tensor
    edge_idx: torch.Tensor
    sub: torch.Tensor
    mapping: torch.Tensor
    pairs: torch.Tensor

    @property
    def n_mov(self) -> int:
        return int(self.mov.shape[0])

    @property
    def n_sc(self) -> int:
        return int(self.edge_idx.shape[0])


def sidechain_rotate_mask(m: int, sub, mapping) -> np.ndarray:
    """bool [n_sc, m]: row j marks the atoms bond j turns (the [n_sc, m] rotate mask of the subcomponents)."""
    sub, mapping = np.asarray(sub, dtype=np.int64).reshape(-1), np.asarray(mapping, dtype=np.int64).reshape(-1, 2)
    mask = np.zeros((mapping.shape[0], m), dtype=bool)
    for j, (a, b) in enumerate(mapping.tolist()):
        mask[j, sub[a:b]] = True
    return mask


def build_sc_pairs(m: int, nbrs, rotate_mask, mov) -> torch.Tensor:
    """uint8 [n_mov, m]: row r lists the partners b of atom a = mov[r] in sc(y): b != a, more than 3 bonds from a in the bond graph
    `nbrs` (neighbour lists; no path counts as far) and rotate_mask[j][a] != rotate_mask[j][b] for some bond j.  This is the rule of
    refine.build_self_pairs(m, bonds, rotate_mask), read per moving atom: row r holds (pairs | pairs.T)[mov[r]].  A pair of two moving
    atoms therefore appears in both rows."""
    mask = np.asarray(rotate_mask, dtype=bool).reshape(-1, m)
    mov = np.asarray(mov, dtype=np.int64).reshape(-1)
    out = np.zeros((len(mov), m), dtype=np.uint8)
    for r, a in enumerate(mov.tolist()):
        near, front = {a}, {a}
        for _ in range(3):
            front = {c for b in front for c in nbrs[b]} - near
            near |= front
        split = (mask != mask[:, a:a + 1]).any(0) if mask.shape[0] else np.zeros(m, dtype=bool)
        split[list(near)] = False
        out[r] = split
    return torch.from_numpy(out)


def receptor_bonds(graph) -> list:
    """Neighbour lists of the receptor bond graph: scoring.distance_bonds on the graph's own atom positions."""
    x = torch.as_tensor(graph["atom"].x).long().numpy()
    z = np.array([ATOMIC_NUMS[i] if ATOMIC_NUMS[i] != "misc" else 0 for i in x[:, 1].tolist()], dtype=np.int64)
    return distance_bonds(torch.as_tensor(graph["atom"].pos).double().numpy(), z)


def sidechain_tables(graph) -> Optional[SidechainTables]:
    """SidechainTables of a complex graph, checked on the host (indices inside the atom nodes, mapping inside the subcomponents, no
    atom twice in one bond's subcomponent); None for a graph without flexResidues."""
    if "flexResidues" not in graph or len(graph["flexResidues"]) == 0:
        return None
    fr = graph["flexResidues"]
    m = int(graph["atom"].pos.shape[0])
    edge = torch.as_tensor(fr.edge_idx).long().reshape(-1, 2).cpu()
    sub = torch.as_tensor(fr.subcomponents).long().reshape(-1).cpu()
    mapping = torch.as_tensor(fr.subcomponentsMapping).long().reshape(-1, 2).cpu()
    check_sidechain_tables(m, edge, sub, mapping)
    mov = torch.unique(sub)
    pairs = build_sc_pairs(m, receptor_bonds(graph), sidechain_rotate_mask(m, sub, mapping), mov)
    return SidechainTables(mov, edge, sub, mapping, pairs)


def check_sidechain_tables(m: int, edge, sub, mapping, mov=None):
    """Raises ValueError unless the side-chain tables are consistent with m receptor atoms (what the device skips, it is never handed)."""
    if mapping.shape[0] != edge.shape[0]:
        raise ValueError(f"subcomponentsMapping has {mapping.shape[0]} rows for {edge.shape[0]} side-chain bonds")
    for name, t in (("flexResidues.edge_idx", edge), ("flexResidues.subcomponents", sub)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= m):
            raise ValueError(f"{name}: atom index outside [0, {m})")
    if mapping.numel() and (int(mapping.min()) < 0 or int(mapping.max()) > sub.numel() or bool((mapping[:, 0] > mapping[:, 1]).any())):
        raise ValueError("subcomponentsMapping: a range outside the subcomponents")
    for a, b in mapping.tolist():
        if len(set(sub[a:b].tolist())) != b - a:
            raise ValueError("flexResidues.subcomponents: an atom twice in one bond's subcomponent")
    if mov is not None:
        mv = torch.as_tensor(mov).long().reshape(-1)
        if mv.numel() and (int(mv.min()) < 0 or int(mv.max()) >= m or bool((mv[1:] <= mv[:-1]).any())):
            raise ValueError(f"mov: sorted unique atom indices inside [0, {m})")
        if not set(sub.tolist()) <= set(mv.tolist()):
            raise ValueError("flexResidues.subcomponents: an atom outside the moving set")


# ---------------------------------------------------------------------------------------------- the PyTorch fp64 form
def _tables(ra, fa, rb, fb):
    ok = (ra[:, None] >= 0) & (rb[None, :] >= 0)
    hyd = (fa[:, None] & fb[None, :] & 1) != 0
    hb = ((((fa[:, None] >> 1) & (fb[None, :] >> 2)) | ((fa[:, None] >> 2) & (fb[None, :] >> 1))) & 1) != 0
    return ra[:, None] + rb[None, :], ok, hyd, hb


def energy_flex_torch(x, y, x0, y0, lig_r, lig_f, rec_r, rec_f, self_pairs, mov, sc_pairs, config: ScoreConfig, restraint: float = 0.0,
                      restraint_sc: float = 0.0):
    """([S, 6] fp64 = inter, intra, sc, ligand restraint term, side-chain restraint term, E; [S, n, 3] fp64 dE/dx; [S, n_mov, 3] fp64
    dE/dy over the moving atoms) of fp32 poses x [S, n, 3] and receptors y [S, m, 3] against the start (x0, y0) - the definition of the
    module docstring on host tensors.  mov [n_mov] int64, sc_pairs uint8 [n_mov, m]."""
    c = config
    S, n = x.shape[0], x.shape[1]
    n_mov = int(mov.shape[0])
    e7, gx = score_torch(x, lig_r, lig_f, y, rec_r, rec_f, self_pairs, c, 1.0, with_grad=True)
    dx = x.double() - x0.double()
    rest = restraint * dx.pow(2).sum(-1).mean(-1)
    gx = gx + (2.0 * restraint / n) * dx
    sc = torch.zeros(S, dtype=torch.float64)
    rest_sc = torch.zeros(S, dtype=torch.float64)
    gy = torch.zeros(S, n_mov, 3, dtype=torch.float64)
    if n_mov:
        x64, y64 = x.double(), y.double()
        ym = y64[:, mov]
        lr, rr = lig_r.double(), rec_r.double()
        lf, rf = lig_f.to(torch.int64), rec_f.to(torch.int64)
        # d inter / dy_a by gather: the moving atom first, the ligand atoms second
        _, g_inter = _pair_sums(ym[:, :, None, :] - x64[:, None, :, :], *_tables(rr[mov], rf[mov], lr, lf), c, True)
        # sc: partners that are static count once, partners that move are met from both ends and count half each time
        rs, ok, hyd, hb = _tables(rr[mov], rf[mov], rr, rf)
        is_mov = torch.zeros(y.shape[1], dtype=torch.bool)
        is_mov[mov] = True
        diff = ym[:, :, None, :] - y64[:, None, :, :]
        t_st, g_st = _pair_sums(diff, rs, ok & sc_pairs.bool() & ~is_mov[None, :], hyd, hb, c, True)
        t_mv, g_mv = _pair_sums(diff, rs, ok & sc_pairs.bool() & is_mov[None, :], hyd, hb, c, True)
        sc = _weighted(t_st + 0.5 * t_mv, c)
        dy = ym - y0.double()[:, mov]
        rest_sc = restraint_sc * dy.pow(2).sum(-1).mean(-1)
        gy = g_inter + g_st + g_mv + (2.0 * restraint_sc / n_mov) * dy
    e = torch.stack([e7[:, 4], e7[:, 5], sc, rest, rest_sc, (((e7[:, 4] + e7[:, 5]) + sc) + rest) + rest_sc], 1)
    return e, gx, gy


def direction_sc_torch(y, gy, mov, edge_idx, sub, mapping):
    """fp64 d_sc [S, n_sc] of the module docstring (not yet multiplied by the step); gy [S, n_mov, 3] over the moving atoms `mov`."""
    y = y.double()
    S, m = y.shape[0], y.shape[1]
    g = torch.zeros(S, m, 3, dtype=torch.float64)
    g[:, mov] = gy
    zero = torch.zeros((), dtype=torch.float64)
    d = torch.zeros(S, edge_idx.shape[0], dtype=torch.float64)
    for j in range(edge_idx.shape[0]):
        u, v = int(edge_idx[j, 0]), int(edge_idx[j, 1])
        idx = sub[int(mapping[j, 0]):int(mapping[j, 1])]
        idx = idx[(idx != u) & (idx != v)]                     # the bond's own atoms lie on the axis: no lever, exactly
        axis = y[:, u] - y[:, v]
        axis = axis / axis.norm(dim=-1, keepdim=True)
        a = torch.cross(axis[:, None, :].expand(-1, idx.shape[0], -1), y[:, idx] - y[:, v:v + 1], dim=-1)
        num, dn = (g[:, idx] * a).sum((1, 2)), a.pow(2).sum((1, 2))
        d[:, j] = torch.where(dn == 0, zero, -num / dn)
    return d


def descend_flex_torch(E, x0, y0, step, acc, iterations, config, bonds, mask_rotate, rot_idx, ref_lig, sc: SidechainTables, history=None):
    """The CPU fp64 loop: descent.descend_torch with the receptor in the state.  E(x [S, n, 3] fp32, y [S, m, 3] fp32) -> (e [S, 6] fp64
    with the total in column 5, gx, gy); start state x0, y0, step [S] fp64, acc [S] int32 (none is modified); the ligand tables as
    descend_torch takes them.  Returns (x, y, step, acc, e0, e)."""
    c = config
    T = int(bonds.shape[0])
    x, y = x0.clone(), y0.clone()
    e, gx, gy = E(x, y)
    e0 = e.clone()
    if history is not None:
        history.append(e[:, 5].clone())
    for _ in range(iterations if x.shape[0] else 0):
        d_tr, d_rot, d_tor = direction_torch(x, gx, bonds, mask_rotate)
        d_sc = direction_sc_torch(y, gy, sc.mov, sc.edge_idx, sc.sub, sc.mapping)
        # a sample without a finite energy can never accept: it goes through the ligand update as descend_torch sends it
        fin = torch.isfinite(e[:, 5])
        tr, rot, tor, scs = (torch.where(fin[:, None], step[:, None] * d, torch.zeros_like(d)).float() for d in (d_tr, d_rot, d_tor, d_sc))
        xt = modify_conformer(torch.where(fin[:, None, None], x, ref_lig[None]), tr, rot, tor if T else None, bonds, rot_idx)
        yt = apply_sidechain_torsions(y, sc.edge_idx, sc.sub, sc.mapping, scs) if sc.n_sc else y
        et, gxt, gyt = E(xt, yt)
        take = et[:, 5] < e[:, 5]                      # strict, fp64; False for NaN
        x = torch.where(take[:, None, None], xt, x)
        y = torch.where(take[:, None, None], yt, y)
        gx = torch.where(take[:, None, None], gxt, gx)
        gy = torch.where(take[:, None, None], gyt, gy)
        e = torch.where(take[:, None], et, e)
        step = torch.where(take, (c.step_grow * step).clamp(max=c.step_max), c.step_shrink * step)
        acc = acc + take.to(torch.int32)
        if history is not None:
            history.append(e[:, 5].clone())
    return x, y, step, acc, e0, e


# ---------------------------------------------------------------------------------------------- the class
class FlexPoseMinimizer:
    """Joint minimisation of the poses of one complex and their flexible side chains (see the module docstring).

    graph, device, score_config: as PoseMinimizer with receptor="graph" (the moving atoms are the graph's atom nodes); config: a
    MinimizeConfig, whose `sidechain_restraint` is k_sc.  A graph without flexResidues is handed to PoseMinimizer unchanged: minimize
    and advance then return what PoseMinimizer returns."""

    def __init__(self, graph, device="cpu", score_config: Optional[ScoreConfig] = None, config: Optional[MinimizeConfig] = None):
        self.rigid = PoseMinimizer(graph, device, "graph", score_config, config)
        self.config, self.device, self.scorer, self.score_config = self.rigid.config, self.rigid.device, self.rigid.scorer, self.rigid.score_config
        if not (self.config.sidechain_restraint >= 0):
            raise ValueError("MinimizeConfig: sidechain_restraint must not be negative")
        self.n, self.n_a = self.rigid.n, self.rigid.n_a
        self.sc = sidechain_tables(graph)
        self._ref_rec = torch.as_tensor(graph["atom"].pos).float().reshape(-1, 3)
        if self.sc is not None and self.device.type != "cpu":
            from . import launch as LA
            self._sc_dev = LA.flex_tables(self.sc, self.n_a, self.device)      # checked on the host, uploaded once

    @property
    def flexible(self) -> bool:
        return self.sc is not None

    def fused_available(self) -> bool:
        """Whether ligand and side chains fit the kernel's limits."""
        return self._limit() is None

    def _limit(self) -> Optional[str]:
        from . import _lib as L
        r = self.rigid
        if r.n > L.DDP_MINIMIZE_MAX_ATOMS or r.T > L.DDP_MINIMIZE_MAX_TORSIONS:
            return f"DDP_MINIMIZE_MAX_ATOMS = {L.DDP_MINIMIZE_MAX_ATOMS}, DDP_MINIMIZE_MAX_TORSIONS = {L.DDP_MINIMIZE_MAX_TORSIONS}"
        if self.sc.n_mov > L.DDP_MINIMIZE_FLEX_MAX_MOVING:
            return f"DDP_MINIMIZE_FLEX_MAX_MOVING = {L.DDP_MINIMIZE_FLEX_MAX_MOVING}"
        if self.sc.n_sc > L.DDP_MINIMIZE_FLEX_MAX_BONDS:
            return f"DDP_MINIMIZE_FLEX_MAX_BONDS = {L.DDP_MINIMIZE_FLEX_MAX_BONDS}"
        if L.flex_state_bytes(r.n, self.sc.n_mov, self.sc.n_sc) > L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES:
            return f"DDP_MINIMIZE_FLEX_MAX_STATE_BYTES = {L.DDP_MINIMIZE_FLEX_MAX_STATE_BYTES}"
        return None

    def _rec(self, x, atom_pos):
        self.rigid._check(x, atom_pos)
        if atom_pos is None:
            return self._ref_rec.to(x.device)[None].repeat(x.shape[0], 1, 1).contiguous()
        return atom_pos.float().contiguous()

    def _E(self, x0, y0):
        t, c, sc = self.scorer._cpu, self.config, self.sc
        return lambda x, y: energy_flex_torch(x, y, x0, y0, t["lig_r"], t["lig_f"], t["rec_r"], t["rec_f"], t["pairs"], sc.mov, sc.pairs,
                                              self.score_config, c.restraint, c.sidechain_restraint)

    # ---- energy
    def energy(self, lig_pos, atom_pos=None, anchor=None, atom_anchor=None):
        """([S, 6] fp64 energies, [S, n, 3] fp64 dE/dx, [S, n_mov, 3] fp64 dE/dy over the moving atoms); anchors None: the state itself.
        A graph without flexResidues: PoseMinimizer.energy."""
        if not self.flexible:
            return self.rigid.energy(lig_pos, anchor, atom_pos)
        x, y = lig_pos.float().contiguous(), self._rec(lig_pos, atom_pos)
        x0 = x if anchor is None else anchor.float().contiguous()
        y0 = y if atom_anchor is None else atom_anchor.float().contiguous()
        if x0.shape != x.shape or y0.shape != y.shape or x0.device != x.device or y0.device != x.device:
            raise ValueError("anchors: the shapes and device of the state")
        S = x.shape[0]
        if not x.is_cuda:
            return self._E(x0, y0)(x, y)
        if not self.fused_available():
            return tuple(t.to(x.device) for t in self._E(x0.cpu(), y0.cpu())(x.cpu(), y.cpu()))
        with torch.cuda.device(x.device):
            step = torch.zeros(S, dtype=torch.float64, device=x.device)
            acc = torch.zeros(S, dtype=torch.int32, device=x.device)
            gx = torch.empty(S, self.n, 3, dtype=torch.float64, device=x.device)
            gy = torch.empty(S, self.sc.n_mov, 3, dtype=torch.float64, device=x.device)
            e = self._run_fused(x, y, x0, y0, step, acc, 0, None, gx, gy)[4]
        return e, gx, gy

    # ---- minimisation
    def minimize(self, lig_pos, atom_pos=None, history: Optional[List[torch.Tensor]] = None):
        """Runs config.iterations iterations on lig_pos [S, n, 3] and atom_pos [S, m, 3] (None: the graph's own atoms for every sample)
        and returns a FlexMinimizeResult on the poses' device; no input is modified.  history: as PoseMinimizer.minimize.  A graph
        without flexResidues: PoseMinimizer.minimize and its MinimizeResult."""
        if not self.flexible:
            return self.rigid.minimize(lig_pos, atom_pos, history)
        c = self.config
        x0, y0 = lig_pos.float().contiguous(), self._rec(lig_pos, atom_pos)
        S = x0.shape[0]
        step = torch.full((S,), float(c.step_init), dtype=torch.float64, device=x0.device)
        acc = torch.zeros(S, dtype=torch.int32, device=x0.device)
        x, y, _, acc, e0, e1 = self.advance(x0, y0, x0, y0, step, acc, c.iterations, history)
        moved = (x.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt().float()
        mov = self.sc.mov.to(x.device)
        sc_moved = (y[:, mov].double() - y0[:, mov].double()).pow(2).sum(-1).mean(-1).sqrt().float()
        return FlexMinimizeResult(x, y, e0, e1, self.scorer.score(x0, y0), self.scorer.score(x, y), moved, sc_moved, acc)

    def advance(self, lig_pos, atom_pos, anchor, atom_anchor, step, accepted, iterations: int, history=None):
        """`iterations` iterations from an explicit state: poses lig_pos [S, n, 3] and receptors atom_pos [S, m, 3] fp32, their starts
        `anchor` and `atom_anchor`, step [S] fp64, accepted [S] int32.  Returns (poses, receptors, step, accepted, energy_in [S, 6],
        energy_out [S, 6]) as new tensors; no argument is modified.  A run of a + b iterations equals advance(a) followed by advance(b)
        on the state returned (the device form: bit for bit).  A graph without flexResidues: PoseMinimizer.advance (atom_anchor unused)."""
        if not self.flexible:
            return self.rigid.advance(lig_pos, anchor, step, accepted, iterations, atom_pos, history)
        x, y = lig_pos.float().contiguous(), self._rec(lig_pos, atom_pos)
        x0, y0 = anchor.float().contiguous(), atom_anchor.float().contiguous()
        if x0.shape != x.shape or y0.shape != y.shape or x0.device != x.device or y0.device != x.device:
            raise ValueError("anchors: the shapes and device of the state")
        S = x.shape[0]
        if tuple(step.shape) != (S,) or tuple(accepted.shape) != (S,) or step.device != x.device or accepted.device != x.device:
            raise ValueError("step, accepted: one entry per pose, on the poses' device")
        if iterations < 0:
            raise ValueError("iterations must not be negative")
        step, accepted = step.to(torch.float64).clone(), accepted.to(torch.int32).clone()
        if x.is_cuda and self.fused_available():
            with torch.cuda.device(x.device):
                return self._run_fused(x, y, x0, y0, step, accepted, iterations, history, None, None)
        dev = x.device
        if x.is_cuda:
            _warn_once(f"FlexPoseMinimizer: {self.n} ligand atoms, {self.sc.n_mov} moving atoms, {self.sc.n_sc} side-chain bonds exceed the "
                       f"kernel's limits ({self._limit()}): running the CPU form on host copies")
            x, y, x0, y0, step, accepted = (t.cpu() for t in (x, y, x0, y0, step, accepted))
        r = self.rigid
        h = [] if history is not None else None
        out = descend_flex_torch(self._E(x0, y0), x, y, step, accepted, iterations, self.config, r.bonds, r.mask_rotate, r.rot_idx,
                                 r._ref_lig, self.sc, h)
        if history is not None:
            history.extend(t.to(dev) for t in h)
        return tuple(t.to(dev) for t in out)

    def _run_fused(self, x0, y0, anchor, atom_anchor, step, acc, iterations, history, grad, grad_mov):
        from . import launch as LA
        c, r = self.config, self.rigid
        S = x0.shape[0]
        t = self.scorer._dev
        x, y = x0.clone(), y0.clone()
        e0 = torch.empty(S, 6, dtype=torch.float64, device=x.device)
        e1 = torch.empty(S, 6, dtype=torch.float64, device=x.device)
        h = torch.empty(iterations + 1, S, dtype=torch.float64, device=x.device) if history is not None else None
        LA.pose_minimize_flex(x, anchor, t["lig_r"], t["lig_f"], y, atom_anchor, t["rec_r"], t["rec_f"], self.score_config, t["pairs"],
                              r._bonds_i32 if r.T else None, r._mask_u8 if r.T else None, self._sc_dev, step, acc, e0, e1, iterations,
                              restraint=c.restraint, restraint_sc=c.sidechain_restraint, grow=c.step_grow, shrink=c.step_shrink,
                              step_max=c.step_max, history=h, grad=grad, grad_mov=grad_mov)
        if history is not None:
            history.extend(h.unbind(0))
        return x, y, step, acc, e0, e1
