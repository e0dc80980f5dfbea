"""Monte Carlo search around the sampled poses in the Vinardo-form score of scoring.py: iterated local search (random move, local
descent, Metropolis decision, as in Vina's outer loop).  minimize.py descends from the sampled pose and stays in its basin; here every
sampled pose seeds R independent replicas that each walk over several basins and keep the lowest minimum they have seen.  This
docstring is the definition; include/ddp_hip.h, csrc/ddp_search.hip and DESIGN 4.24 refer to it.

For poses x0[s], s < S, with R replicas each, row q = s R + r.  All arithmetic is that of minimize.py on the same energy, fp64 on the
fp32 inputs, with the sampled pose as the anchor of every replica (k = 0 by default):

    E(x) = inter(x) + intra(x) + k * mean_i |x_i - x0[s]_i|^2

State of a row: the current pose xc with its energies ec[4] (inter, intra, restraint term, E), the best pose xb with eb[4], best_cycle,
and the number of accepted descent trials.  Fresh state: xc = xb = x0[s], every entry of ec and eb +inf, best_cycle = -1, accepted = 0.

Cycle c (global index, counted from 0 over all calls) of row q:
  1. Start pose.  start = pose_update(xc, perturb[c][q]), the sampler's pose map (sampler.modify_conformer / ddp_pose_update), fp32;
     perturb[c][q] has 6 + T fp32 entries: tr, rot, then the torsions in bond order.  Replica 0 at cycle 0 is the exception: start = xc
     bit for bit and its perturb entries are ignored.
  2. Descent.  K iterations of the minimiser's line search (descent.py) from start, with step = step_init; grow, shrink and cap are
     MinimizeConfig's.  It gives the local minimum xl with el[4]; E_start is the energy before the first iteration.
  3. Metropolis.  move = (el[3] < ec[3]) or (u[c][q] < exp(-(el[3] - ec[3]) / temperature)), in fp64.  A NaN makes both comparisons
     false; the first cycle of a row with a finite el always moves, since ec[3] = +inf.  On a move xc = xl, ec = el.
  4. Best.  If el[3] < eb[3] (strict) then xb = xl, eb = el, best_cycle = c.
  5. Record.  trace[c][q] = (E_start, el[3]); flags[c][q] = move | improved << 1; accepted[q] += the accepted trials of the descent.

Selection per pose: the replica with the smallest eb[3], compared with strict < in replica order from replica 0: ties go to the lower
replica; NaN or +inf is never smaller; if every replica is at +inf, replica 0 is chosen, whose xb is the sampled pose.

Replica 0 starts with a plain descent from the sampled pose, so the result is never worse in E than PoseMinimizer's with the same
iteration count: energy_after[:, 3] <= energy_minimized[:, 3] <= energy_before[:, 3] holds exactly, not within a tolerance.

The random numbers are inputs, not device state: perturb [C][S R][6 + T] fp32 and u [C][S R] fp64 in [0, 1) are drawn here from a CPU
torch.Generator seeded with SearchConfig.seed, in a fixed order (randn for perturb, then rand for u), scaled by sigma_tr, sigma_rot and
sigma_tor, and uploaded once.  Every form sees the same numbers and a run is reproducible from its seed.  A SearchState carries the
numbers of all config.cycles cycles, so advance(a) followed by advance(b) equals advance(a + b).

What it is not:
  - not Vina's search: all degrees of freedom move at once, and the local step is the line search of descent.py, not BFGS;
  - no side-chain or receptor motion here: this class searches flexible rows against each sample's own, fixed side chains.  The
    search that moves the side chains with the ligand is search_flex.py (SearchConfig.sidechains, FlexPoseSearcher);
  - no hydrogens;
  - the score is not validated against smina or Vina (see scoring.py), so a lower E is not a better pose;
  - no exchange between replicas (no parallel tempering).

Three forms of the same algorithm, as in minimize.py:
  - CPU tensors: per cycle sampler.modify_conformer for the move and descent.descend_torch (through PoseMinimizer.advance) over the
    S R rows, torch.where for the decisions.  This form is the definition.
  - device tensors, fused=True: csrc/ddp_search.hip.  ddp_pose_search runs all cycles of all rows in ONE launch of S R workgroups
    (the minimiser alone fills S of the chip's 256 CUs, so up to 256 rows the replicas run beside each other), ddp_pose_search_select
    picks the replica.  The descent of a cycle is the loop of ddp_pose_minimize, bit for bit.
  - device tensors, fused=False: per cycle modify_conformer_hip, PoseMinimizer.advance(fused=False) and torch.where; it never
    synchronises.  It is the timing baseline and the path of ligands above the fused kernel's limits (DDP_MINIMIZE_MAX_ATOMS,
    DDP_MINIMIZE_MAX_TORSIONS): fused=True falls back to it there, with a one-time warning that names the limit.  It is not bit-equal
    to the fused form: the pose maps differ in their block sums, as documented for the minimiser.
Between the forms a decision whose two sides agree to the last bits may fall differently, after which the chains differ; every form
on its own obeys the inequality above."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import torch

from .minimize import MinimizeConfig, PoseMinimizer, _warn_once
from .sampler import modify_conformer, modify_conformer_hip
from .scoring import PoseScorer, PoseScores, ScoreConfig


@dataclass
class SearchConfig:
    """The constants of the search.  Untuned choices, not fitted to anything; the step constants of the descent are MinimizeConfig's
    defaults."""
    replicas: int = 6             # R, independent chains per sampled pose
    cycles: int = 10              # C, cycles per chain
    iterations: int = 30          # K, line-search iterations of one descent
    temperature: float = 1.2      # of the Metropolis rule, in units of E
    sigma_tr: float = 1.0         # standard deviation of the random translation, A per axis
    sigma_rot: float = 0.3        # of the random rotation vector, rad per axis
    sigma_tor: float = 0.5        # of the random torsion steps, rad per bond
    seed: int = 0                 # of the CPU generator that draws perturb and u
    restraint: float = 0.0        # k of the restraint to the sampled pose
    sidechains: bool = False      # run_csv: flexible rows go through search_flex.FlexPoseSearcher (PoseSearcher ignores it)
    sigma_chi: float = 0.3        # search_flex.py: standard deviation of the random side-chain steps, rad per bond
    sidechain_restraint: float = 0.0   # k_sc of search_flex.py, the restraint of the moving side-chain atoms to their sampled positions


@dataclass
class SearchState:
    """The rows' state after `cycle` cycles, with the random numbers of all cycles (see the module docstring)."""
    x0: torch.Tensor               # [S, n, 3] fp32 the sampled poses
    cur_pos: torch.Tensor          # [S R, n, 3] fp32
    cur_e: torch.Tensor            # [S R, 4] fp64
    best_pos: torch.Tensor         # [S R, n, 3] fp32
    best_e: torch.Tensor           # [S R, 4] fp64
    best_cycle: torch.Tensor       # [S R] int32
    accepted: torch.Tensor         # [S R] int32
    perturb: torch.Tensor          # [C, S R, 6 + T] fp32
    u: torch.Tensor                # [C, S R] fp64
    trace: torch.Tensor            # [C, S R, 2] fp64, rows >= cycle not yet written
    flags: torch.Tensor            # [C, S R] uint8
    energy_minimized: torch.Tensor  # [S, 4] fp64: ec of replica 0 after cycle 0 (+inf before, and where the pose has no finite energy)
    cycle: int = 0                 # cycles done


@dataclass
class SearchResult:
    """Per-sample results of PoseSearcher.search, in the order of the poses handed in, on their device."""
    lig_pos: torch.Tensor          # [S, n, 3] fp32 the best pose of the chosen replica
    energy_before: torch.Tensor    # [S, 4] fp64: inter, intra, restraint term, E of the sampled pose
    energy_minimized: torch.Tensor  # [S, 4] after the plain descent of replica 0 in cycle 0
    energy_after: torch.Tensor     # [S, 4] of lig_pos
    scores_before: PoseScores      # PoseScorer.score of the poses handed in: `total` is comparable with scores.csv
    scores_after: PoseScores       # PoseScorer.score of lig_pos
    replica: torch.Tensor          # [S] int32 the chosen replica
    cycle: torch.Tensor            # [S] int32 the cycle in which it found lig_pos (-1: never left the sampled pose)
    moves: torch.Tensor            # [S] int32 Metropolis moves of the chosen replica
    rmsd_moved: torch.Tensor       # [S] fp32 plain RMSD between the input and lig_pos
    trace: torch.Tensor            # [C, S R, 2] fp64 (E_start, E of the local minimum) of every cycle and row
    flags: torch.Tensor            # [C, S R] uint8 move | improved << 1

    def cpu(self) -> "SearchResult":
        return SearchResult(**{k: v.cpu() for k, v in self.__dict__.items()})

    def index(self, order) -> "SearchResult":
        return index_result(self, order)


def index_result(result, order):
    """A SearchResult or FlexSearchResult with the samples `order`: per-sample fields by sample, trace and flags by the samples' rows."""
    S = result.lig_pos.shape[0]
    R = result.trace.shape[1] // S if S else 1
    out = {}
    for k, v in result.__dict__.items():
        if isinstance(v, PoseScores):
            out[k] = v.index(order)
        elif k in ("trace", "flags"):
            o = order.to(v.device).long()
            out[k] = v[:, (o[:, None] * R + torch.arange(R, device=v.device)[None]).reshape(-1)]
        else:
            out[k] = v[order.to(v.device)]
    return type(result)(**out)


def check_config(c: SearchConfig, sidechains: bool = False):
    """Raises ValueError for constants no search can run with; sidechains: sigma_chi and sidechain_restraint are looked at too."""
    if c.replicas < 1 or c.cycles < 0 or c.iterations < 0:
        raise ValueError("SearchConfig: replicas must be at least 1, cycles and iterations must not be negative")
    if not (c.temperature > 0) or c.temperature == float("inf"):
        raise ValueError("SearchConfig: temperature must be positive and finite")
    own = ((c.sidechain_restraint,), (c.sigma_chi,)) if sidechains else ((), ())
    if not all(k >= 0 for k in (c.restraint,) + own[0]) or min(c.sigma_tr, c.sigma_rot, c.sigma_tor, *own[1]) < 0:
        raise ValueError("SearchConfig: the restraints and the sigmas must not be negative" if sidechains else
                         "SearchConfig: restraint and the sigmas must not be negative")


def draw_random_numbers(config: SearchConfig, rows: int, T: int, n_sc: int = 0):
    """(perturb [C, rows, 6 + T + n_sc] fp32, u [C, rows] fp64) of the module docstring (n_sc > 0: of search_flex.py's), on the host: one
    generator, randn then rand; the four blocks of perturb scaled by sigma_tr, sigma_rot, sigma_tor and sigma_chi."""
    gen = torch.Generator().manual_seed(int(config.seed))
    perturb = torch.randn(config.cycles, rows, 6 + T + n_sc, generator=gen, dtype=torch.float32)
    u = torch.rand(config.cycles, rows, generator=gen, dtype=torch.float64)
    perturb[..., 0:3] *= float(config.sigma_tr)
    perturb[..., 3:6] *= float(config.sigma_rot)
    perturb[..., 6:6 + T] *= float(config.sigma_tor)
    perturb[..., 6 + T:] *= float(config.sigma_chi)
    return perturb.contiguous(), u.contiguous()


def per_row(t, R: int):
    """[S, ...] -> [S R, ...]: every pose's entry once per replica, in row order (a copy; no synchronisation on any device)."""
    return t[:, None].expand(t.shape[0], R, *t.shape[1:]).reshape(t.shape[0] * R, *t.shape[1:])


def select_rows(best_e, best_cycle, R: int, *coords):
    """The selection rule with tensor operations (any device, no synchronisation) on the last entry of best_e: (the rows of every tensor
    of coords, energy [S, .], replica [S] int32, cycle [S] int32).  argmin returns the first of equal values: the lower replica; NaN and
    +inf count as +inf."""
    S = best_e.shape[0] // R
    e = best_e[:, -1].reshape(S, R)
    key = torch.where(e < float("inf"), e, torch.full_like(e, float("inf")))
    rep = key.argmin(1) if S else torch.zeros(0, dtype=torch.int64, device=best_e.device)
    q = torch.arange(S, device=best_e.device) * R + rep
    return [t[q].clone() for t in coords], best_e[q].clone(), rep.to(torch.int32), best_cycle[q].clone()


def select_torch(best_e, best_pos, best_cycle, R: int):
    """select_rows for the rigid state: (pos [S, n, 3], energy [S, 4], replica [S] int32, cycle [S] int32)."""
    (pos,), e, rep, cyc = select_rows(best_e, best_cycle, R, best_pos)
    return pos, e, rep, cyc


class PoseSearcher:
    """The search around the poses of one complex (see the module docstring).

    graph, device, receptor, score_config, scorer: as PoseMinimizer.  One PoseMinimizer is built (iterations = config.iterations,
    restraint = config.restraint, the default step constants) and its tables are reused.

    The chain driver below (the fresh state, advance with its clone / early-out / "cycle 0 is a launch of its own" logic, steps 3 to 5
    of a cycle, what a result derives from a state) serves search_flex.FlexPoseSearcher too: a state is the sampled input, the
    coordinate tensors cur_X / best_X for X in _COORDS, which are always taken or kept together, and _WIDTH energies with the total
    last."""
    _State, _COORDS, _WIDTH = SearchState, ("pos",), 4

    def __init__(self, graph, device="cpu", receptor=None, score_config: Optional[ScoreConfig] = None,
                 config: Optional[SearchConfig] = None, scorer: Optional[PoseScorer] = None):
        c = self.config = config or SearchConfig()
        check_config(c)
        self.minimizer = PoseMinimizer(graph, device, receptor=receptor, score_config=score_config, scorer=scorer,
                                       config=MinimizeConfig(iterations=c.iterations, restraint=c.restraint))
        self.device = self.minimizer.device
        self.scorer = self.minimizer.scorer
        self.n, self.T = self.minimizer.n, self.minimizer.T
        self._ref_lig = self.minimizer._ref_lig.to(self.device)      # uploaded once: the cycles never synchronise

    @property
    def _rigid(self) -> PoseMinimizer:
        """The minimiser that holds the ligand's torsion tables."""
        return self.minimizer

    # ---- state
    def _fresh(self, sampled: dict, coords, n_sc: int = 0):
        """The fresh state: sampled = the inputs (x0 [S, n, 3] first), coords = the rows' coordinates in the order of _COORDS, with the
        random numbers of config.cycles cycles on the poses' device."""
        c, W = self.config, self._WIDTH
        x0 = sampled["x0"]
        S, dev = x0.shape[0], x0.device
        rows = S * c.replicas
        perturb, u = draw_random_numbers(c, rows, self.T, n_sc)
        if dev.type != "cpu":          # from pinned memory: the upload does not synchronise
            perturb, u = (t.pin_memory().to(dev, non_blocking=True) for t in (perturb, u))
        inf = float("inf")
        f64 = dict(dtype=torch.float64, device=dev)
        kw = {p + k: (t if p == "cur_" else t.clone()) for k, t in zip(self._COORDS, coords) for p in ("cur_", "best_")}
        return self._State(**sampled, **kw, cur_e=torch.full((rows, W), inf, **f64), best_e=torch.full((rows, W), inf, **f64),
                           best_cycle=torch.full((rows,), -1, dtype=torch.int32, device=dev),
                           accepted=torch.zeros(rows, dtype=torch.int32, device=dev), perturb=perturb, u=u,
                           trace=torch.full((c.cycles, rows, 2), float("nan"), **f64),
                           flags=torch.zeros(c.cycles, rows, dtype=torch.uint8, device=dev), energy_minimized=torch.full((S, W), inf, **f64),
                           cycle=0)

    def start(self, lig_pos, atom_pos=None) -> SearchState:
        """The fresh state of lig_pos [S, n, 3] with the random numbers of config.cycles cycles on the poses' device."""
        self.minimizer._check(lig_pos, atom_pos)
        x0 = lig_pos.float().contiguous().clone()
        return self._fresh(dict(x0=x0), [per_row(x0, self.config.replicas).contiguous()])

    def _advance(self, state, cycles: int, fused: bool, run_fused, cycle):
        """`cycles` further cycles on a copy of `state`: run_fused(st, a, b) runs the cycles a ... b - 1 in one launch, cycle(st, c) one
        cycle with tensor operations."""
        R = self.config.replicas
        c0, c1 = state.cycle, state.cycle + int(cycles)
        if cycles < 0 or c1 > state.u.shape[0]:
            raise ValueError(f"advance: {cycles} cycles from cycle {c0}, the state carries the random numbers of {state.u.shape[0]}")
        moving = [p + k for k in self._COORDS + ("e",) for p in ("cur_", "best_")]
        st = replace(state, **{k: getattr(state, k).clone() for k in moving + ["best_cycle", "accepted", "trace", "flags", "energy_minimized"]})
        st.cycle = c1
        if cycles == 0 or state.x0.shape[0] == 0:
            return st
        if fused:
            with torch.cuda.device(state.x0.device):
                if c0 == 0:      # cycle 0 is a launch of its own: the state between it and cycle 1 holds energy_minimized
                    run_fused(st, 0, 1)
                    st.energy_minimized = st.cur_e[::R].clone()
                if c1 > max(c0, 1):
                    run_fused(st, max(c0, 1), c1)
        else:
            for cyc in range(c0, c1):
                cycle(st, cyc)
        return st

    def advance(self, state: SearchState, cycles: int, atom_pos=None, fused: bool = True, starts=None) -> SearchState:
        """`cycles` further cycles on a copy of `state` (which is not modified): cycles state.cycle ... state.cycle + cycles - 1 with the
        state's own random numbers.  advance(a) followed by advance(b) equals advance(a + b) (the fused form: bit for bit).  starts: a
        list that receives the [S R, n, 3] start pose of every cycle run (device tensors, no synchronisation)."""
        mz = self.minimizer
        mz._check(state.x0, atom_pos)
        if not state.x0.is_cuda:
            fused = False
        elif fused and cycles > 0 and state.x0.shape[0] and not mz.fused_available():
            from . import _lib as L
            _warn_once(f"PoseSearcher: {self.n} ligand atoms / {self.T} rotatable bonds exceed the fused kernel's limits "
                       f"(DDP_MINIMIZE_MAX_ATOMS = {L.DDP_MINIMIZE_MAX_ATOMS}, DDP_MINIMIZE_MAX_TORSIONS = {L.DDP_MINIMIZE_MAX_TORSIONS}): "
                       "running cycle by cycle, launch by launch")
            fused = False
        return self._advance(state, cycles, fused, lambda st, a, b: self._run_fused(st, a, b, atom_pos, starts),
                             lambda st, cyc: self._cycle(st, cyc, atom_pos, starts))

    def _run_fused(self, st: SearchState, a: int, b: int, atom_pos, starts):
        from . import launch as LA
        c, mz = self.config, self.minimizer
        t, rec = mz._tables(st.x0, atom_pos)
        mc = mz.config
        so = torch.empty(b - a, st.cur_pos.shape[0], self.n, 3, dtype=torch.float32, device=st.x0.device) if starts is not None else None
        LA.pose_search(st.x0, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], mz.score_config, t["pairs"],
                       mz._bonds_i32 if self.T else None, mz._mask_u8 if self.T else None, c.replicas, a, st.perturb[a:b], st.u[a:b],
                       st.cur_pos, st.cur_e, st.best_pos, st.best_e, st.best_cycle, st.accepted, st.trace[a:b], st.flags[a:b],
                       c.iterations, c.temperature, step_init=mc.step_init, restraint=c.restraint, grow=mc.step_grow, shrink=mc.step_shrink,
                       step_max=mc.step_max, starts=so)
        if starts is not None:
            starts.extend(so.unbind(0))

    def _start_pose(self, st, cyc: int, fin):
        """Step 1 for the ligand of all rows: (p, keep, start) = the cycle's move, the rows that start where they are and the start pose.
        A row without finite coordinates (fin false) goes through the pose map as the graph's own pose with a zero move (its NaNs never
        reach the batched SVD of the alignment) and then starts from its own pose: its energy is NaN, it never moves."""
        mz, T, dev, xc = self._rigid, self.T, st.x0.device, st.cur_pos
        p = torch.where(fin[:, None], st.perturb[cyc], torch.zeros_like(st.perturb[cyc]))
        src = torch.where(fin[:, None, None], xc, self._ref_lig.to(dev)[None])
        tor = p[:, 6:6 + T].contiguous() if T else None
        if dev.type == "cpu":
            moved = modify_conformer(src, p[:, 0:3], p[:, 3:6], tor, mz.bonds, mz.rot_idx)
        else:
            moved = modify_conformer_hip(src, p[:, 0:3], p[:, 3:6], tor, mz._bonds_i32, mz._mask_u8)
        keep = ~fin
        if cyc == 0:
            keep = keep | (torch.arange(xc.shape[0], device=dev) % self.config.replicas == 0)
        return p, keep, torch.where(keep[:, None, None], xc, moved).contiguous()

    def _descent_step(self, rows: int, dev):
        """(step, accepted) every descent of a cycle starts with."""
        return (torch.full((rows,), float(self.minimizer.config.step_init), dtype=torch.float64, device=dev),
                torch.zeros(rows, dtype=torch.int32, device=dev))

    def _decide(self, st, cyc: int, minimum, taken, e_start, el):
        """Steps 3 to 5 of a cycle on all rows with tensor operations: 3. Metropolis, 4. best, 5. record.  minimum: the local minimum's
        coordinates in the order of _COORDS; el, e_start: its energies and the start state's."""
        R = self.config.replicas
        d = el[:, -1] - st.cur_e[:, -1]
        move = (el[:, -1] < st.cur_e[:, -1]) | (st.u[cyc] < torch.exp(-d / self.config.temperature))
        improved = el[:, -1] < st.best_e[:, -1]
        for k, xl in zip(self._COORDS, minimum):
            setattr(st, "cur_" + k, torch.where(move[:, None, None], xl, getattr(st, "cur_" + k)))
            setattr(st, "best_" + k, torch.where(improved[:, None, None], xl, getattr(st, "best_" + k)))
        st.cur_e = torch.where(move[:, None], el, st.cur_e)
        st.best_e = torch.where(improved[:, None], el, st.best_e)
        st.best_cycle = torch.where(improved, torch.full_like(st.best_cycle, cyc), st.best_cycle)
        st.accepted = st.accepted + taken
        st.trace[cyc, :, 0], st.trace[cyc, :, 1] = e_start[:, -1], el[:, -1]
        st.flags[cyc] = move.to(torch.uint8) | (improved.to(torch.uint8) << 1)
        if cyc == 0:
            st.energy_minimized = st.cur_e[::R].clone()

    def _cycle(self, st: SearchState, cyc: int, atom_pos, starts):
        """One cycle of all rows with tensor operations: the CPU form, and the launch-by-launch device form (it never synchronises)."""
        R = self.config.replicas
        _, _, start = self._start_pose(st, cyc, torch.isfinite(st.cur_pos).all(2).all(1))
        if starts is not None:
            starts.append(start)
        step, zero = self._descent_step(start.shape[0], start.device)
        ap = None if atom_pos is None else per_row(atom_pos, R)
        xl, _, taken, e_start, el = self.minimizer.advance(start, per_row(st.x0, R), step, zero, self.config.iterations, ap, fused=False)
        self._decide(st, cyc, [xl], taken, e_start, el)

    # ---- results
    def select(self, state: SearchState, fused: bool = True):
        """(pos [S, n, 3], energy [S, 4], replica [S], cycle [S]) of the state by the selection rule."""
        R = self.config.replicas
        if state.x0.is_cuda and fused and state.x0.shape[0]:
            from . import launch as LA
            with torch.cuda.device(state.x0.device):
                return LA.pose_search_select(state.best_pos, state.best_e, state.best_cycle, R)
        return select_torch(state.best_e, state.best_pos, state.best_cycle, R)

    def _summary(self, state, e_before, e_after, pos, rep):
        """What a result derives from a state and its selection: (energy_minimized, energy_after, moves [S] int32, rmsd_moved [S]
        fp32).  A state without a cycle (config.cycles = 0) gives the sampled state back: the identity."""
        x0, e_min = state.x0, state.energy_minimized
        S = x0.shape[0]
        if state.cycle == 0:
            e_after, e_min = e_before.clone(), e_before.clone()
        q = torch.arange(S, device=x0.device) * self.config.replicas + rep.long()
        moves = (state.flags[:state.cycle, q] & 1).sum(0).to(torch.int32) if S else torch.zeros(0, dtype=torch.int32, device=x0.device)
        return e_min, e_after, moves, (pos.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt().float()

    def result(self, state: SearchState, atom_pos=None, fused: bool = True) -> SearchResult:
        """The SearchResult of a state.  A state without a cycle (config.cycles = 0) gives the sampled poses back: the identity."""
        x0 = state.x0
        e_before = self.minimizer.energy(x0, atom_pos=atom_pos)[0] if x0.shape[0] else torch.zeros(0, 4, dtype=torch.float64, device=x0.device)
        pos, e_after, rep, cyc = self.select(state, fused)
        e_min, e_after, moves, moved = self._summary(state, e_before, e_after, pos, rep)
        return SearchResult(pos, e_before, e_min, e_after, self.scorer.score(x0, atom_pos), self.scorer.score(pos, atom_pos), rep, cyc, moves,
                            moved, state.trace, state.flags)

    def search(self, lig_pos, atom_pos=None, fused: bool = True) -> SearchResult:
        """Runs config.cycles cycles of config.replicas replicas on lig_pos [S, n, 3] (flexible runs: atom_pos [S, n_a, 3], each sample's
        own static receptor) and returns a SearchResult on the poses' device.  The input tensor is not modified.  fused: device tensors
        only, see the module docstring."""
        state = self.advance(self.start(lig_pos, atom_pos), self.config.cycles, atom_pos, fused)
        return self.result(state, atom_pos, fused)
