"""Monte Carlo search around the sampled poses TOGETHER with the flexible side chains of their receptor: the search of search.py on
the joint energy of minimize_flex.py.  search.py walks the ligand around side chains frozen at their sampled rotamers; here the chi
angles of the flexible residues take part in the random move and in the local descent, as Vina's flexible residues do.  This docstring
states what differs from search.py, whose definition (the cycle, the Metropolis rule, the selection, the random numbers, the three
forms) and whose chain driver hold here; include/ddp_hip.h, csrc/ddp_search_flex.hip and DESIGN 4.26 refer to both.

For poses x0[s], s < S, with the receptor atoms y0[s] (atom_pos[s], each sample's own) and R replicas each, row q = s R + r.  Mv, the
moving set, and the side-chain tables are minimize_flex.py's (n_mov atoms, n_sc bonds).  All arithmetic is that of minimize_flex.py
on the same energy, fp64 on the fp32 inputs, with the sampled state (x0[s], y0[s]) as the anchor of every replica (k = k_sc = 0 by
default):

    E(x, y) = inter(x, y) + intra(x) + sc(y) + k mean_i |x_i - x0[s]_i|^2 + k_sc mean_{a in Mv} |y_a - y0[s]_a|^2

with six entries: inter, intra, sc, ligand restraint term, side-chain restraint term, E.  Every decision is taken on entry 5.

State of a row: that of search.py with, beside every ligand pose (xc, xb), the moving atoms ymc, ymb [n_mov, 3] (the atoms of Mv only,
in the order of Mv; every other receptor atom is y0[s] and never changes) and six energies.  Fresh state: ymc = ymb = y0[s][Mv].  x
and y are always taken or kept together.

Cycle c of row q, where it differs:
  1. Start state.  perturb[c][q] has 6 + T + n_sc fp32 entries: tr, rot, the ligand torsions in bond order, then one angle per
     side-chain bond in list order (scaled by sigma_chi; with n_sc = 0 these are exactly the numbers of search.py).  The ligand goes
     through the pose map as in search.py; the moving atoms go through the side-chain map (sampler.apply_sidechain_torsions /
     ddp_sidechain_update: bonds in list order, fp32, no re-alignment) applied to y0[s] with ymc in place of its moving atoms.
     Replica 0 at cycle 0 starts at the sampled state bit for bit.
  2. Descent.  K iterations of the joint line search (minimize_flex.descend_flex_torch / the loop of ddp_pose_minimize_flex).
  3. to 5. as search.py, on entry 5 of the energies.

Replica 0 starts with a plain joint descent from the sampled state, so the result is never worse in E than FlexPoseMinimizer's with
the same iteration count: energy_after[:, 5] <= energy_minimized[:, 5] <= energy_before[:, 5] holds exactly.  energy_minimized is ec of
replica 0 after cycle 0, which is FlexPoseMinimizer with K iterations.

What it is not, beyond search.py's list:
  - no backbone motion, and no receptor atom outside the flexible residues moves;
  - no rotamer library: a chi move is a Gaussian step around the current rotamer, so a rotamer far from the sampled one is reached
    only through a chain of accepted moves;
  - sigma_chi is as untuned as the other constants.

The forms: the CPU form moves with sampler.modify_conformer and sampler.apply_sidechain_torsions and descends with
FlexPoseMinimizer.advance over the S R rows; fused=True is csrc/ddp_search_flex.hip, ONE launch of S R workgroups on the LDS plan of
ddp_pose_minimize_flex, whose loop a cycle's descent is bit for bit, with the selection by select_flex_torch on the device (a copy of S
rows, no synchronisation); fused=False on the device runs modify_conformer_hip, apply_sidechain_torsions_hip and one launch of
ddp_pose_minimize_flex per cycle.  Above the limits of ddp_pose_minimize_flex (DDP_MINIMIZE_FLEX_MAX_MOVING,
DDP_MINIMIZE_FLEX_MAX_BONDS, DDP_MINIMIZE_FLEX_MAX_STATE_BYTES and the ligand limits) the class does what FlexPoseMinimizer does: it
warns once, naming the limit, and runs the CPU form on host copies.  A graph without flexible residues raises: that is PoseSearcher's
case."""
from __future__ import annotations

from dataclasses import dataclass, fields, replace
from typing import Optional

import torch

from .minimize import MinimizeConfig, _warn_once
from .minimize_flex import FlexPoseMinimizer
from .sampler import apply_sidechain_torsions, apply_sidechain_torsions_hip
from .scoring import PoseScores, ScoreConfig
from .search import PoseSearcher, SearchConfig, check_config, draw_random_numbers, index_result, per_row, select_rows

draw_random_numbers_flex = draw_random_numbers      # (config, rows, T, n_sc)


@dataclass
class FlexSearchState:
    """The rows' state after `cycle` cycles, with the random numbers of all cycles (see the module docstring)."""
    x0: torch.Tensor               # [S, n, 3] fp32 the sampled poses
    y0: torch.Tensor               # [S, m, 3] fp32 the sampled receptors
    cur_pos: torch.Tensor          # [S R, n, 3] fp32
    cur_mov: torch.Tensor          # [S R, n_mov, 3] fp32
    cur_e: torch.Tensor            # [S R, 6] fp64
    best_pos: torch.Tensor         # [S R, n, 3] fp32
    best_mov: torch.Tensor         # [S R, n_mov, 3] fp32
    best_e: torch.Tensor           # [S R, 6] fp64
    best_cycle: torch.Tensor       # [S R] int32
    accepted: torch.Tensor         # [S R] int32
    perturb: torch.Tensor          # [C, S R, 6 + T + n_sc] fp32
    u: torch.Tensor                # [C, S R] fp64
    trace: torch.Tensor            # [C, S R, 2] fp64, rows >= cycle not yet written
    flags: torch.Tensor            # [C, S R] uint8
    energy_minimized: torch.Tensor  # [S, 6] fp64: ec of replica 0 after cycle 0 (+inf before, and where the state has no finite energy)
    cycle: int = 0                 # cycles done


@dataclass
class FlexSearchResult:
    """Per-sample results of FlexPoseSearcher.search, in the order of the poses handed in, on their device."""
    lig_pos: torch.Tensor                # [S, n, 3] fp32 the best pose of the chosen replica
    atom_pos: torch.Tensor               # [S, m, 3] fp32 the receptor atoms with that replica's best side chains
    energy_before: torch.Tensor          # [S, 6] fp64: inter, intra, sc, ligand restraint term, side-chain restraint term, E
    energy_minimized: torch.Tensor       # [S, 6] after the plain joint descent of replica 0 in cycle 0
    energy_after: torch.Tensor           # [S, 6] of (lig_pos, atom_pos)
    scores_before: PoseScores            # PoseScorer.score of the poses handed in against the side chains handed in
    scores_after: PoseScores             # PoseScorer.score of lig_pos against atom_pos, its own searched side chains
    replica: torch.Tensor                # [S] int32 the chosen replica
    cycle: torch.Tensor                  # [S] int32 the cycle in which it found the state (-1: never left the sampled state)
    moves: torch.Tensor                  # [S] int32 Metropolis moves of the chosen replica
    rmsd_moved: torch.Tensor             # [S] fp32 plain RMSD between the input and lig_pos
    sidechain_rmsd_moved: torch.Tensor   # [S] fp32 the same over the moving atoms Mv
    trace: torch.Tensor                  # [C, S R, 2] fp64 (E_start, E of the local minimum) of every cycle and row
    flags: torch.Tensor                  # [C, S R] uint8 move | improved << 1

    def cpu(self) -> "FlexSearchResult":
        return FlexSearchResult(**{k: v.cpu() for k, v in self.__dict__.items()})

    def index(self, order) -> "FlexSearchResult":
        return index_result(self, order)


def select_flex_torch(best_e, best_pos, best_mov, best_cycle, R: int):
    """search.select_rows for the joint state: (pos [S, n, 3], mov [S, n_mov, 3], energy [S, 6], replica [S] int32, cycle [S] int32)."""
    (pos, mov), e, rep, cyc = select_rows(best_e, best_cycle, R, best_pos, best_mov)
    return pos, mov, e, rep, cyc


class FlexPoseSearcher(PoseSearcher):
    """The search around the poses of one complex with its flexible side chains (see the module docstring): the chain driver of
    PoseSearcher on the joint state.

    graph, device, score_config: as FlexPoseMinimizer.  One FlexPoseMinimizer is built (iterations = config.iterations, restraint =
    config.restraint, sidechain_restraint = config.sidechain_restraint, the default step constants) and its tables are reused."""
    _State, _COORDS, _WIDTH = FlexSearchState, ("pos", "mov"), 6

    def __init__(self, graph, device="cpu", score_config: Optional[ScoreConfig] = None, config: Optional[SearchConfig] = None):
        c = self.config = config or SearchConfig(sidechains=True)
        check_config(c, sidechains=True)
        self.minimizer = FlexPoseMinimizer(graph, device, score_config,
                                           MinimizeConfig(iterations=c.iterations, restraint=c.restraint,
                                                          sidechain_restraint=c.sidechain_restraint))
        if not self.minimizer.flexible:
            raise ValueError("FlexPoseSearcher: the graph has no flexible residues (flexResidues); search rigid rows with PoseSearcher")
        self._bind()

    def _bind(self):
        """The attributes derived from self.minimizer (a FlexPoseMinimizer with side-chain tables)."""
        mz = self.minimizer
        self.device, self.scorer, self.sc = mz.device, mz.scorer, mz.sc
        self.n, self.T = mz.rigid.n, mz.rigid.T
        self.n_mov, self.n_sc = mz.sc.n_mov, mz.sc.n_sc
        self._ref_lig = mz.rigid._ref_lig.to(self.device)            # uploaded once: the cycles never synchronise
        self._mov = mz.sc.mov.to(self.device)

    @property
    def _rigid(self):
        return self.minimizer.rigid

    # ---- state
    def start(self, lig_pos, atom_pos=None) -> FlexSearchState:
        """The fresh state of lig_pos [S, n, 3] and atom_pos [S, m, 3] (None: the graph's own atoms for every sample) with the random
        numbers of config.cycles cycles on the poses' device."""
        R = self.config.replicas
        x0 = lig_pos.float().contiguous().clone()
        y0 = self.minimizer._rec(lig_pos, atom_pos).clone()
        coords = [per_row(x0, R).contiguous(), per_row(y0[:, self._mov.to(x0.device)], R).contiguous()]
        return self._fresh(dict(x0=x0, y0=y0), coords, self.n_sc)

    def advance(self, state: FlexSearchState, cycles: int, fused: bool = True, starts=None) -> FlexSearchState:
        """`cycles` further cycles on a copy of `state` (which is not modified): cycles state.cycle ... state.cycle + cycles - 1 with the
        state's own random numbers.  advance(a) followed by advance(b) equals advance(a + b) (the fused form: bit for bit).  starts: a
        list that receives (start pose [S R, n, 3], start moving atoms [S R, n_mov, 3]) of every cycle run."""
        mz, dev = self.minimizer, state.x0.device
        if state.x0.is_cuda and cycles > 0 and state.x0.shape[0] and not mz.fused_available():
            _warn_once(f"FlexPoseSearcher: {self.n} ligand atoms, {self.n_mov} moving atoms, {self.n_sc} side-chain bonds exceed the "
                       f"kernel's limits ({mz._limit()}): running the CPU form on host copies")
            tensors = [f.name for f in fields(state) if f.name != "cycle"]
            hs = [] if starts is not None else None
            host = self.advance(replace(state, **{k: getattr(state, k).cpu() for k in tensors}), cycles, False, hs)
            if starts is not None:
                starts.extend((a.to(dev), b.to(dev)) for a, b in hs)
            return replace(host, **{k: getattr(host, k).to(dev) for k in tensors})
        return self._advance(state, cycles, fused and state.x0.is_cuda, lambda st, a, b: self._run_fused(st, a, b, starts),
                             lambda st, cyc: self._cycle(st, cyc, starts))

    def _run_fused(self, st: FlexSearchState, a: int, b: int, starts):
        from . import launch as LA
        c, mz = self.config, self.minimizer
        r, mc, t = mz.rigid, mz.config, mz.scorer._dev
        rows, dev = st.cur_pos.shape[0], st.x0.device
        so = torch.empty(b - a, rows, self.n, 3, dtype=torch.float32, device=dev) if starts is not None else None
        sm = torch.empty(b - a, rows, self.n_mov, 3, dtype=torch.float32, device=dev) if starts is not None else None
        LA.pose_search_flex(st.x0, t["lig_r"], t["lig_f"], st.y0, t["rec_r"], t["rec_f"], mz.score_config, t["pairs"],
                            r._bonds_i32 if r.T else None, r._mask_u8 if r.T else None, mz._sc_dev, c.replicas, a, st.perturb[a:b], st.u[a:b],
                            st.cur_pos, st.cur_mov, st.cur_e, st.best_pos, st.best_mov, st.best_e, st.best_cycle, st.accepted, st.trace[a:b],
                            st.flags[a:b], c.iterations, c.temperature, step_init=mc.step_init, restraint=c.restraint,
                            restraint_sc=c.sidechain_restraint, grow=mc.step_grow, shrink=mc.step_shrink, step_max=mc.step_max, starts=so,
                            starts_mov=sm)
        if starts is not None:
            starts.extend(zip(so.unbind(0), sm.unbind(0)))

    def _cycle(self, st: FlexSearchState, cyc: int, starts):
        """One cycle of all rows with tensor operations: the CPU form, and the launch-by-launch device form (it never synchronises)."""
        mz, sc = self.minimizer, self.minimizer.sc
        R, dev = self.config.replicas, st.x0.device
        mov = self._mov.to(dev)
        x0r, y0r = per_row(st.x0, R), per_row(st.y0, R)
        yc = y0r.clone()
        yc[:, mov] = st.cur_mov
        # 1. the start state: the ligand as in search.py (a NaN in a moving atom keeps the row where it is too), then the side chains
        p, keep, start_x = self._start_pose(st, cyc, torch.isfinite(st.cur_pos).all(2).all(1) & torch.isfinite(st.cur_mov).all(2).all(1))
        chi = p[:, 6 + self.T:].contiguous()
        if not self.n_sc:
            ymoved = yc
        elif dev.type == "cpu":
            ymoved = apply_sidechain_torsions(yc, sc.edge_idx, sc.sub, sc.mapping, chi)
        else:
            d = mz._sc_dev
            ymoved = apply_sidechain_torsions_hip(yc, d["edge_idx"], d["sub"], d["mapping"], chi)
        start_y = torch.where(keep[:, None, None], yc, ymoved).contiguous()
        if starts is not None:
            starts.append((start_x, start_y[:, mov].contiguous()))
        # 2. the descent, then 3. to 5. on (x, y[Mv])
        step, zero = self._descent_step(start_x.shape[0], dev)
        xl, yl, _, taken, e_start, el = mz.advance(start_x, start_y, x0r, y0r, step, zero, self.config.iterations)
        self._decide(st, cyc, [xl, yl[:, mov]], taken, e_start, el)

    # ---- results
    def select(self, state: FlexSearchState):
        """(pos [S, n, 3], mov [S, n_mov, 3], energy [S, 6], replica [S], cycle [S]) of the state by the selection rule."""
        return select_flex_torch(state.best_e, state.best_pos, state.best_mov, state.best_cycle, self.config.replicas)

    def result(self, state: FlexSearchState) -> FlexSearchResult:
        """The FlexSearchResult of a state.  A state without a cycle (config.cycles = 0) gives the sampled state back: the identity."""
        x0, y0 = state.x0, state.y0
        S, dev = x0.shape[0], x0.device
        e_before = self.minimizer.energy(x0, y0)[0] if S else torch.zeros(0, 6, dtype=torch.float64, device=dev)
        pos, ym, e_after, rep, cyc = self.select(state)
        mov = self._mov.to(dev)
        y = y0.clone()
        y[:, mov] = ym
        e_min, e_after, moves, moved = self._summary(state, e_before, e_after, pos, rep)
        if self.n_mov:
            sc_moved = (ym.double() - y0[:, mov].double()).pow(2).sum(-1).mean(-1).sqrt().float()
        else:
            sc_moved = torch.zeros(S, dtype=torch.float32, device=dev)
        return FlexSearchResult(pos, y, e_before, e_min, e_after, self.scorer.score(x0, y0), self.scorer.score(pos, y), rep, cyc, moves, moved,
                                sc_moved, state.trace, state.flags)

    def search(self, lig_pos, atom_pos=None, fused: bool = True) -> FlexSearchResult:
        """Runs config.cycles cycles of config.replicas replicas on lig_pos [S, n, 3] and atom_pos [S, m, 3] (None: the graph's own atoms
        for every sample) and returns a FlexSearchResult on the poses' device.  No input is modified.  fused: device tensors only, see
        the module docstring."""
        return self.result(self.advance(self.start(lig_pos, atom_pos), self.config.cycles, fused))
