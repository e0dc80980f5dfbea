"""Local minimisation of sampled poses in the Vinardo-form score of scoring.py, then rescoring: the step that follows sampling in a
docking pipeline.  The clash relief of refine.py can only push atoms apart; this descends the whole score (attraction, hydrophobic
and hydrogen-bond terms included) along the sampler's own degrees of freedom, so bond lengths, angles and rings cannot change.

Energy of one pose x against the pose x0 it started from, fp64 on the fp32 inputs (converted first):

    E(x) = inter(x) + intra(x) + k * mean_i |x_i - x0_i|^2

inter and intra are scoring.py's, exactly: the same ScoreConfig, typing, cutoff, self pairs and NaN rule; they are NOT divided by the
torsion divisor.  Gradient: scoring.py's d(inter + intra)/dx plus (2 k / n)(x - x0).  Default k = 0.

The search direction and the backtracking line search with its strict accept rule are those of descent.py, which states them, shared
with the clash relief: the trial is modify_conformer(x, step d_tr, step d_rot, step d_tor), its fp32 arguments rounded from fp64 as
ddp_refine_direction rounds them.  MinimizeConfig holds the constants; they are untuned choices.

What it does not do:
  - no receptor or side-chain motion: flexible rows are minimised against each sample's own, fixed side chains (the joint form,
    in which the chi angles of the flexible residues descend with the ligand, is minimize_flex.py);
  - no hydrogens;
  - no global search: it is a local descent from the sampled pose (search.py runs Monte Carlo moves around it, each followed by
    this descent);
  - the score is not validated against smina or Vina (see scoring.py), so neither is its minimum: on the 3dpf fixture the crystal
    pose itself moves 0.47 A and goes from E = -10.97 to -13.65, the score's minimum is NOT the crystal pose;
  - E is only C0 at the kinks of the ramps and has a jump of about 1e-11 at the cutoff; the pose map re-aligns the conformer after
    the torsions, so d_tor is not the exact derivative of the map that is applied.  The accept rule, not the gradient, is what
    guarantees that E never rises.

Three forms of the same algorithm:
  - CPU tensors: descent.descend_torch on the fp64 energy below, built on scoring.score_torch.  This form is the definition.
  - device tensors, fused=True: csrc/ddp_minimize.hip (ddp_pose_minimize), one workgroup per pose runs all iterations in ONE launch.
  - device tensors, fused=False: descent.descend_hip, launch by launch from the existing entries (ddp_pose_score with its gradient and
    a few elementwise torch operations for the restraint as the evaluation); it never synchronises.  It is the timing
    baseline and the path of ligands above the fused kernel's limits (DDP_MINIMIZE_MAX_ATOMS atoms, DDP_MINIMIZE_MAX_TORSIONS
    rotatable bonds): fused=True falls back to it there, with a one-time warning that names the limit.
The device forms follow the CPU form up to rounding: a trial whose energy equals the current one to the last bits may be accepted by
one form and rejected by another, after which the step sequences differ; every form on its own never lets E rise."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import List, Optional

import torch

from .descent import DescentBuffers, descend_hip, descend_torch, ligand_torsions
from .pose_args import check_anchor
from .sampler import rotate_index_lists
from .scoring import PoseScorer, PoseScores, ScoreConfig, score_torch


@dataclass
class MinimizeConfig:
    """The constants of the line search.  Untuned choices, not fitted to anything."""
    iterations: int = 100         # fixed number of iterations
    restraint: float = 0.0        # k of the restraint to the start pose
    step_init: float = 1.0        # first step size of every pose
    step_grow: float = 2.0        # factor after an accepted trial
    step_shrink: float = 0.5      # factor after a rejected trial
    step_max: float = 1024.0      # cap of the step size
    sidechains: bool = False      # run_csv: flexible rows go through minimize_flex.FlexPoseMinimizer (PoseMinimizer ignores it)
    sidechain_restraint: float = 0.0   # k_sc of minimize_flex.py, the restraint of the moving side-chain atoms to their start


@dataclass
class MinimizeResult:
    """Per-sample results of PoseMinimizer.minimize, in the order of the poses handed in, on their device."""
    lig_pos: torch.Tensor          # [S, n, 3] fp32 minimised poses
    energy_before: torch.Tensor    # [S, 4] fp64: inter, intra, restraint term, E
    energy_after: torch.Tensor     # [S, 4]
    scores_before: PoseScores      # PoseScorer.score of the poses handed in: `total` is comparable with scores.csv
    scores_after: PoseScores       # PoseScorer.score of lig_pos
    rmsd_moved: torch.Tensor       # [S] fp32 plain RMSD between the input and the minimised pose
    accepted: torch.Tensor         # [S] int32 accepted trials

    def cpu(self) -> "MinimizeResult":
        return MinimizeResult(**{k: v.cpu() for k, v in self.__dict__.items()})

    def index(self, order) -> "MinimizeResult":
        return MinimizeResult(**{k: (v.index(order) if isinstance(v, PoseScores) else v[order.to(v.device)]) for k, v in self.__dict__.items()})


def energy_torch(x, anchor, lig_r, lig_f, rec, rec_r, rec_f, self_pairs, config: ScoreConfig, restraint: float = 0.0):
    """([S, 4] fp64 = inter, intra, restraint term, E; [S, n, 3] fp64 gradient) of fp32 poses x against `anchor` - the definition of the
    module docstring on host tensors."""
    e7, g = score_torch(x, lig_r, lig_f, rec, rec_r, rec_f, self_pairs, config, 1.0, with_grad=True)
    dx = x.double() - anchor.double()
    rest = restraint * dx.pow(2).sum(-1).mean(-1)
    g = g + (2.0 * restraint / x.shape[1]) * dx
    return torch.stack([e7[:, 4], e7[:, 5], rest, e7[:, 4] + e7[:, 5] + rest], 1), g


_warned = set()


def _warn_once(msg: str):
    if msg not in _warned:
        _warned.add(msg)
        warnings.warn(msg, stacklevel=3)


class PoseMinimizer:
    """Minimisation of the poses of one complex in the physics score (see the module docstring).

    graph, device, receptor, score_config: as PoseScorer - receptor None or "graph" (the graph's atom nodes; each sample's own atom_pos
    when one is handed in: flexible runs) or a scoring.TypedReceptor in the graph's frame.  One PoseScorer is built and its tables are
    reused.  scorer: a PoseScorer of the same graph on the same device, in place of receptor and score_config: its tables and config
    are used and none is built."""

    def __init__(self, graph, device="cpu", receptor=None, score_config: Optional[ScoreConfig] = None,
                 config: Optional[MinimizeConfig] = None, scorer: Optional[PoseScorer] = None):
        self.config = config or MinimizeConfig()
        if not (self.config.restraint >= 0) or self.config.iterations < 0:
            raise ValueError("MinimizeConfig: restraint and iterations must not be negative")
        self.device = torch.device(device)
        if scorer is None:
            scorer = PoseScorer(graph, device, receptor="graph" if receptor is None else receptor, config=score_config)
        elif receptor is not None or score_config is not None:
            raise ValueError("scorer: given in place of receptor and score_config, not with them")
        elif scorer.device != self.device:
            raise ValueError(f"scorer built for {scorer.device}, minimiser for {self.device}")
        self.scorer = scorer
        self.score_config = self.scorer.config
        self.n, self.n_a = self.scorer.n, self.scorer.n_a
        self.bonds, self.mask_rotate = ligand_torsions(graph)
        self.T = int(self.bonds.shape[0])
        self.rot_idx = rotate_index_lists(self.mask_rotate)
        self._ref_lig = torch.as_tensor(graph["ligand"].pos).float().reshape(-1, 3)
        if self.device.type != "cpu":
            from . import launch as LA
            self._bonds_i32 = LA.refine_bonds(self.bonds, self.n, self.device)      # checked on the host, uploaded once
            self._mask_u8 = self.mask_rotate.to(torch.uint8).contiguous().to(self.device)

    # ---- checks and tables
    def _check(self, lig_pos, atom_pos):
        self.scorer._check(lig_pos, atom_pos)

    def _tables(self, x, atom_pos):
        t = self.scorer._dev if x.is_cuda else self.scorer._cpu
        rec = atom_pos.float().contiguous() if (atom_pos is not None and self.scorer.receptor_from_graph) else t["rec"]
        return t, rec

    def fused_available(self) -> bool:
        """Whether the ligand fits the fused kernel's limits."""
        from . import _lib as L
        return self.n <= L.DDP_MINIMIZE_MAX_ATOMS and self.T <= L.DDP_MINIMIZE_MAX_TORSIONS

    # ---- energy
    def energy(self, lig_pos, anchor=None, atom_pos=None):
        """([S, 4] fp64 = inter, intra, restraint term, E; [S, n, 3] fp64 gradient) of the poses; anchor None: the poses themselves."""
        self._check(lig_pos, atom_pos)
        x = lig_pos.float().contiguous()
        a = x if anchor is None else anchor.float().contiguous()
        check_anchor(x, a)
        S = x.shape[0]
        if not x.is_cuda:
            t, rec = self._tables(x, atom_pos)
            return energy_torch(x, a, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], t["pairs"], self.score_config, self.config.restraint)
        with torch.cuda.device(x.device):
            step = torch.zeros(S, dtype=torch.float64, device=x.device)
            acc = torch.zeros(S, dtype=torch.int32, device=x.device)
            g = torch.empty(S, self.n, 3, dtype=torch.float64, device=x.device)
            if self.fused_available():
                _, _, _, e, _ = self._run_fused(x, a, atom_pos, step, acc, 0, None, g)
            else:
                e = torch.empty(S, 4, dtype=torch.float64, device=x.device)
                self._score_hip(x, a.double(), atom_pos, torch.empty(S, 7, dtype=torch.float64, device=x.device), g, e)
        return e, g

    # ---- minimisation
    def minimize(self, lig_pos, atom_pos=None, history: Optional[List[torch.Tensor]] = None, fused: bool = True) -> MinimizeResult:
        """Runs config.iterations iterations on lig_pos [S, n, 3] (flexible runs: atom_pos [S, n_a, 3], each sample's own static
        receptor) and returns a MinimizeResult on the poses' device.  The input tensor is not modified.  history: a list that receives
        the [S] total energies E before the first and after every iteration (device tensors, no synchronisation).  fused: device
        tensors only, see the module docstring."""
        self._check(lig_pos, atom_pos)
        c = self.config
        x0 = lig_pos.float().contiguous()
        S = x0.shape[0]
        step = torch.full((S,), float(c.step_init), dtype=torch.float64, device=x0.device)
        acc = torch.zeros(S, dtype=torch.int32, device=x0.device)
        x, _, acc, e0, e1 = self.advance(x0, x0, step, acc, c.iterations, atom_pos, history, fused)
        moved = (x.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt().float()
        return MinimizeResult(x, e0, e1, self.scorer.score(x0, atom_pos), self.scorer.score(x, atom_pos), moved, acc)

    def advance(self, lig_pos, anchor, step, accepted, iterations: int, atom_pos=None, history=None, fused: bool = True):
        """`iterations` iterations from an explicit state: poses lig_pos [S, n, 3] fp32, their start poses `anchor`, step [S] fp64,
        accepted [S] int32.  Returns (poses, step, accepted, energy_in [S, 4], energy_out [S, 4]) as new tensors; no argument is
        modified.  A run of a + b iterations equals advance(a) followed by advance(b) on the state returned (the fused form: bit for
        bit)."""
        self._check(lig_pos, atom_pos)
        x = lig_pos.float().contiguous()
        a = anchor.float().contiguous()
        check_anchor(x, a)
        S = x.shape[0]
        if tuple(step.shape) != (S,) or tuple(accepted.shape) != (S,) or step.device != x.device or accepted.device != x.device:
            raise ValueError("step, accepted: one entry per pose, on the poses' device")
        if iterations < 0:
            raise ValueError("iterations must not be negative")
        step, accepted = step.to(torch.float64).clone(), accepted.to(torch.int32).clone()
        c = self.config
        if not x.is_cuda:
            t, rec = self._tables(x, atom_pos)
            return descend_torch(lambda p: energy_torch(p, a, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], t["pairs"], self.score_config,
                                                        c.restraint),
                                 x, step, accepted, iterations, c, self.bonds, self.mask_rotate, self.rot_idx, self._ref_lig, history)
        with torch.cuda.device(x.device):
            if fused and not self.fused_available():
                from . import _lib as L
                _warn_once(f"PoseMinimizer: {self.n} ligand atoms / {self.T} rotatable bonds exceed the fused kernel's limits "
                           f"(DDP_MINIMIZE_MAX_ATOMS = {L.DDP_MINIMIZE_MAX_ATOMS}, DDP_MINIMIZE_MAX_TORSIONS = {L.DDP_MINIMIZE_MAX_TORSIONS}): "
                           "running launch by launch")
                fused = False
            if fused:
                return self._run_fused(x, a, atom_pos, step, accepted, iterations, history, None)
            from . import launch as LA
            t, rec = self._tables(x, atom_pos)
            b, a64 = DescentBuffers(x, self.T), a.double()
            e7 = torch.empty(S, 7, dtype=torch.float64, device=x.device)
            cur = LA.refine_args(b.x, a, t["lig_r"], rec, t["rec_r"], bonds=self._bonds_i32, mask_rotate=self._mask_u8, step=step,
                                 accepted=accepted, grow=c.step_grow, shrink=c.step_shrink, step_max=c.step_max, **b.refine_kwargs())
            x, e0, e1 = descend_hip(lambda pos, e_out, g_out: self._score_hip(pos, a64, atom_pos, e7, g_out, e_out), cur, b, iterations,
                                    self._bonds_i32, self._mask_u8, history)
            return x, step, accepted, e0, e1

    def _run_fused(self, x0, anchor, atom_pos, step, acc, iterations, history, grad):
        from . import launch as LA
        c = self.config
        S = x0.shape[0]
        t, rec = self._tables(x0, atom_pos)
        x = x0.clone()
        e0 = torch.empty(S, 4, dtype=torch.float64, device=x.device)
        e1 = torch.empty(S, 4, dtype=torch.float64, device=x.device)
        h = torch.empty(iterations + 1, S, dtype=torch.float64, device=x.device) if history is not None else None
        LA.pose_minimize(x, anchor, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], self.score_config, t["pairs"],
                         self._bonds_i32 if self.T else None, self._mask_u8 if self.T else None, step, acc, e0, e1, iterations,
                         restraint=c.restraint, grow=c.step_grow, shrink=c.step_shrink, step_max=c.step_max, history=h, grad=grad)
        if history is not None:
            history.extend(h.unbind(0))
        return x, step, acc, e0, e1

    def _score_hip(self, x, anchor64, atom_pos, e7, g, e4):
        """ddp_pose_score of x into e7 and g, then the restraint and E packed into e4 [S, 4] with elementwise torch operations."""
        from . import launch as LA
        t, rec = self._tables(x, atom_pos)
        k = float(self.config.restraint)
        LA.pose_score(x, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], self.score_config, 1.0, t["pairs"], energy=e7, grad=g)
        dx = x.double() - anchor64
        rest = k * dx.pow(2).sum(-1).mean(-1)
        g.add_(dx, alpha=2.0 * k / self.n)
        e4[:, 0], e4[:, 1], e4[:, 2] = e7[:, 4], e7[:, 5], rest
        e4[:, 3] = e7[:, 4] + e7[:, 5] + rest
