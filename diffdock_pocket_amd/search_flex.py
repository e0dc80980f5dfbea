"""Monte Carlo search around the sampled poses TOGETHER with the flexible side chains of their receptor: the search of search.py on
the joint energy of minimize_flex.py.  search.py walks the ligand around side chains frozen at their sampled rotamers; here the chi
angles of the flexible residues take part in the random move and in the local descent, as Vina's flexible residues do.  This docstring
is the definition; include/ddp_hip.h, csrc/ddp_search_flex.hip and DESIGN 4.26 refer to it.

For poses x0[s], s < S, with the receptor atoms y0[s] (atom_pos[s], each sample's own) and R replicas each, row q = s R + r.  Mv, the
moving set, and the side-chain tables are minimize_flex.py's (n_mov atoms, n_sc bonds).  All arithmetic is that of minimize_flex.py
on the same energy, fp64 on the fp32 inputs, with the sampled state (x0[s], y0[s]) as the anchor of every replica (k = k_sc = 0 by
default):

    E(x, y) = inter(x, y) + intra(x) + sc(y) + k mean_i |x_i - x0[s]_i|^2 + k_sc mean_{a in Mv} |y_a - y0[s]_a|^2

with six entries: inter, intra, sc, ligand restraint term, side-chain restraint term, E.  Every decision is taken on entry 5.

State of a row: the current ligand pose xc [n, 3] and the current moving atoms ymc [n_mov, 3] (the atoms of Mv only, in the order of
Mv; every other receptor atom is y0[s] and never changes) with their energies ec[6]; the best state xb, ymb with eb[6]; best_cycle; and
the number of accepted descent trials.  Fresh state: xc = xb = x0[s], ymc = ymb = y0[s][Mv], every entry of ec and eb +inf,
best_cycle = -1, accepted = 0.

Cycle c (global index, counted from 0 over all calls) of row q:
  1. Start state.  perturb[c][q] has 6 + T + n_sc fp32 entries: tr, rot, the ligand torsions in bond order, then one angle per
     side-chain bond in list order.  The ligand goes through the sampler's pose map as in search.py: start_x = pose_update(xc, tr, rot,
     tor).  The moving atoms go through the side-chain map (sampler.apply_sidechain_torsions / ddp_sidechain_update: bonds in list
     order, fp32, no re-alignment) applied to y0[s] with ymc in place of its moving atoms.  Replica 0 at cycle 0 is the exception: it
     starts at the sampled state bit for bit and its perturb entries are ignored.
  2. Descent.  K iterations of the joint line search (minimize_flex.descend_flex_torch / the loop of ddp_pose_minimize_flex) from the
     start state, with step = step_init; grow, shrink and cap are MinimizeConfig's.  It gives the local minimum (xl, yl) with el[6];
     E_start is the energy before the first iteration.
  3. Metropolis.  move = (el[5] < ec[5]) or (u[c][q] < exp(-(el[5] - ec[5]) / temperature)), in fp64; the rule of search.py.  On a
     move xc = xl, ymc = yl[Mv], ec = el: x and y are always taken or kept together.
  4. Best.  If el[5] < eb[5] (strict) then xb = xl, ymb = yl[Mv], eb = el, best_cycle = c.
  5. Record.  trace[c][q] = (E_start, el[5]); flags[c][q] = move | improved << 1; accepted[q] += the accepted trials of the descent.

Selection per pose: the rule of search.py on eb[5].

Replica 0 starts with a plain joint descent from the sampled state, so the result is never worse in E than FlexPoseMinimizer's with
the same iteration count: energy_after[:, 5] <= energy_minimized[:, 5] <= energy_before[:, 5] holds exactly.  energy_minimized is ec of
replica 0 after cycle 0, which is FlexPoseMinimizer with K iterations.

Random numbers: draw_random_numbers_flex draws randn(C, rows, 6 + T + n_sc) and then rand(C, rows) from one CPU generator seeded with
SearchConfig.seed and scales the four blocks by sigma_tr, sigma_rot, sigma_tor and sigma_chi.  With n_sc = 0 these are exactly the
numbers of search.draw_random_numbers.  A state carries the numbers of all config.cycles cycles, so advance(a) followed by advance(b)
equals advance(a + b).

What it is not:
  - no backbone motion, and no receptor atom outside the flexible residues moves;
  - no rotamer library: a chi move is a Gaussian step around the current rotamer, so a rotamer far from the sampled one is reached
    only through a chain of accepted moves;
  - not Vina's search: all degrees of freedom move at once, and the local step is the joint line search, not BFGS;
  - no hydrogens; the constants (sigma_chi among them) are untuned; the score is not validated against smina or Vina, so a lower E
    is not a better pose;
  - no exchange between replicas.

Three forms of the same algorithm:
  - CPU tensors: per cycle sampler.modify_conformer and sampler.apply_sidechain_torsions for the move, descend_flex_torch (through
    FlexPoseMinimizer.advance) over the S R rows, torch.where for the decisions.  This form is the definition.
  - device tensors, fused=True: csrc/ddp_search_flex.hip.  ddp_pose_search_flex runs all cycles of all rows in ONE launch of S R
    workgroups on the LDS plan of ddp_pose_minimize_flex; the descent of a cycle is that kernel's loop, bit for bit.  The selection is
    select_flex_torch on the device (a copy of S rows, no synchronisation).
  - device tensors, fused=False: per cycle modify_conformer_hip, apply_sidechain_torsions_hip, FlexPoseMinimizer.advance (one launch of
    ddp_pose_minimize_flex over the S R rows) and torch.where; it never synchronises.  It is the timing baseline.  It is not bit-equal
    to the fused form, for the reason search.py gives for the rigid pair: the pose maps differ in their block sums.
Above the limits of ddp_pose_minimize_flex (DDP_MINIMIZE_FLEX_MAX_MOVING, DDP_MINIMIZE_FLEX_MAX_BONDS,
DDP_MINIMIZE_FLEX_MAX_STATE_BYTES and the ligand limits) the class does what FlexPoseMinimizer does: it warns once, naming the limit,
and runs the CPU form on host copies.  A graph without flexible residues raises: that is PoseSearcher's case."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import torch

from .minimize import MinimizeConfig, _warn_once
from .minimize_flex import FlexPoseMinimizer
from .sampler import apply_sidechain_torsions, apply_sidechain_torsions_hip, modify_conformer, modify_conformer_hip
from .scoring import PoseScores, ScoreConfig
from .search import SearchConfig, draw_random_numbers, per_row

_STATE = ("cur_pos", "cur_mov", "cur_e", "best_pos", "best_mov", "best_e", "best_cycle", "accepted", "trace", "flags", "energy_minimized")


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
        S = self.lig_pos.shape[0]
        R = self.trace.shape[1] // S if S else 1
        out = {}
        for k, v in self.__dict__.items():
            if isinstance(v, PoseScores):
                out[k] = v.index(order)
            elif k in ("trace", "flags"):
                o = order.to(v.device).long()
                out[k] = v[:, (o[:, None] * R + torch.arange(R, device=v.device)[None]).reshape(-1)]
            else:
                out[k] = v[order.to(v.device)]
        return FlexSearchResult(**out)


def draw_random_numbers_flex(config: SearchConfig, rows: int, T: int, n_sc: int):
    """(perturb [C, rows, 6 + T + n_sc] fp32, u [C, rows] fp64) of the module docstring, on the host: one generator, randn then rand.
    n_sc = 0: exactly search.draw_random_numbers."""
    if n_sc == 0:
        return draw_random_numbers(config, rows, T)
    gen = torch.Generator().manual_seed(int(config.seed))
    perturb = torch.randn(config.cycles, rows, 6 + T + n_sc, generator=gen, dtype=torch.float32)
    u = torch.rand(config.cycles, rows, generator=gen, dtype=torch.float64)
    perturb[..., 0:3] *= float(config.sigma_tr)
    perturb[..., 3:6] *= float(config.sigma_rot)
    perturb[..., 6:6 + T] *= float(config.sigma_tor)
    perturb[..., 6 + T:] *= float(config.sigma_chi)
    return perturb.contiguous(), u.contiguous()


def select_flex_torch(best_e, best_pos, best_mov, best_cycle, R: int):
    """search.select_torch on six energies with the moving atoms (any device, no synchronisation): (pos [S, n, 3], mov [S, n_mov, 3],
    energy [S, 6], replica [S] int32, cycle [S] int32).  argmin returns the first of equal values: the lower replica; NaN and +inf
    count as +inf."""
    S = best_e.shape[0] // R
    e5 = best_e[:, 5].reshape(S, R)
    key = torch.where(e5 < float("inf"), e5, torch.full_like(e5, float("inf")))
    rep = key.argmin(1) if S else torch.zeros(0, dtype=torch.int64, device=best_e.device)
    q = torch.arange(S, device=best_e.device) * R + rep
    return best_pos[q].clone(), best_mov[q].clone(), best_e[q].clone(), rep.to(torch.int32), best_cycle[q].clone()


class FlexPoseSearcher:
    """The search around the poses of one complex with its flexible side chains (see the module docstring).

    graph, device, score_config: as FlexPoseMinimizer.  One FlexPoseMinimizer is built (iterations = config.iterations, restraint =
    config.restraint, sidechain_restraint = config.sidechain_restraint, the default step constants) and its tables are reused."""

    def __init__(self, graph, device="cpu", score_config: Optional[ScoreConfig] = None, config: Optional[SearchConfig] = None):
        c = self.config = config or SearchConfig(sidechains=True)
        if c.replicas < 1 or c.cycles < 0 or c.iterations < 0:
            raise ValueError("SearchConfig: replicas must be at least 1, cycles and iterations must not be negative")
        if not (c.temperature > 0) or c.temperature == float("inf"):
            raise ValueError("SearchConfig: temperature must be positive and finite")
        if not (c.restraint >= 0) or not (c.sidechain_restraint >= 0) or min(c.sigma_tr, c.sigma_rot, c.sigma_tor, c.sigma_chi) < 0:
            raise ValueError("SearchConfig: the restraints and the sigmas must not be negative")
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

    # ---- state
    def start(self, lig_pos, atom_pos=None) -> FlexSearchState:
        """The fresh state of lig_pos [S, n, 3] and atom_pos [S, m, 3] (None: the graph's own atoms for every sample) with the random
        numbers of config.cycles cycles on the poses' device."""
        mz, c = self.minimizer, self.config
        x0 = lig_pos.float().contiguous().clone()
        y0 = mz._rec(lig_pos, atom_pos).clone()
        S, R, dev = x0.shape[0], c.replicas, x0.device
        rows = S * R
        perturb, u = draw_random_numbers_flex(c, rows, self.T, self.n_sc)
        if dev.type != "cpu":          # from pinned memory: the upload does not synchronise
            perturb, u = (t.pin_memory().to(dev, non_blocking=True) for t in (perturb, u))
        inf = float("inf")
        f64 = dict(dtype=torch.float64, device=dev)
        xr = per_row(x0, R).contiguous()
        yr = per_row(y0[:, self._mov.to(dev)], R).contiguous()
        return FlexSearchState(x0, y0, xr, yr, torch.full((rows, 6), inf, **f64), xr.clone(), yr.clone(), torch.full((rows, 6), inf, **f64),
                               torch.full((rows,), -1, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev),
                               perturb, u, torch.full((c.cycles, rows, 2), float("nan"), **f64),
                               torch.zeros(c.cycles, rows, dtype=torch.uint8, device=dev), torch.full((S, 6), inf, **f64), 0)

    def advance(self, state: FlexSearchState, cycles: int, fused: bool = True, starts=None) -> FlexSearchState:
        """`cycles` further cycles on a copy of `state` (which is not modified): cycles state.cycle ... state.cycle + cycles - 1 with the
        state's own random numbers.  advance(a) followed by advance(b) equals advance(a + b) (the fused form: bit for bit).  starts: a
        list that receives (start pose [S R, n, 3], start moving atoms [S R, n_mov, 3]) of every cycle run."""
        c, mz = self.config, self.minimizer
        c0, c1 = state.cycle, state.cycle + int(cycles)
        if cycles < 0 or c1 > state.u.shape[0]:
            raise ValueError(f"advance: {cycles} cycles from cycle {c0}, the state carries the random numbers of {state.u.shape[0]}")
        st = replace(state, **{k: getattr(state, k).clone() for k in _STATE})
        if cycles == 0 or state.x0.shape[0] == 0:
            st.cycle = c1
            return st
        dev = state.x0.device
        if state.x0.is_cuda and not mz.fused_available():
            _warn_once(f"FlexPoseSearcher: {self.n} ligand atoms, {self.n_mov} moving atoms, {self.n_sc} side-chain bonds exceed the "
                       f"kernel's limits ({mz._limit()}): running the CPU form on host copies")
            host = replace(st, **{k: getattr(st, k).cpu() for k in ("x0", "y0", "perturb", "u") + _STATE})
            hs = [] if starts is not None else None
            for cyc in range(c0, c1):
                self._cycle(host, cyc, hs)
            if starts is not None:
                starts.extend((a.to(dev), b.to(dev)) for a, b in hs)
            st = replace(host, **{k: getattr(host, k).to(dev) for k in ("x0", "y0", "perturb", "u") + _STATE})
        elif state.x0.is_cuda and fused:
            with torch.cuda.device(dev):
                if c0 == 0:      # cycle 0 is a launch of its own: the state between it and cycle 1 holds energy_minimized
                    self._run_fused(st, 0, 1, starts)
                    st.energy_minimized = st.cur_e[::c.replicas].clone()
                if c1 > max(c0, 1):
                    self._run_fused(st, max(c0, 1), c1, starts)
        else:
            for cyc in range(c0, c1):
                self._cycle(st, cyc, starts)
        st.cycle = c1
        return st

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
        c, mz = self.config, self.minimizer
        r, sc = mz.rigid, mz.sc
        R, dev, T = c.replicas, st.x0.device, self.T
        rows = st.cur_pos.shape[0]
        mov = self._mov.to(dev)
        xc, ymc = st.cur_pos, st.cur_mov
        x0r, y0r = per_row(st.x0, R), per_row(st.y0, R)
        yc = y0r.clone()
        yc[:, mov] = ymc
        # 1. start state.  A row without finite coordinates goes through the pose map as the graph's own pose with a zero move (its
        # NaNs never reach the batched SVD of the alignment) and then starts from its own state: its energy is NaN, it never moves.
        fin = torch.isfinite(xc).all(2).all(1) & torch.isfinite(ymc).all(2).all(1)
        p = torch.where(fin[:, None], st.perturb[cyc], torch.zeros_like(st.perturb[cyc]))
        src = torch.where(fin[:, None, None], xc, self._ref_lig.to(dev)[None])
        tor = p[:, 6:6 + T].contiguous() if T else None
        chi = p[:, 6 + T:].contiguous()
        if dev.type == "cpu":
            moved = modify_conformer(src, p[:, 0:3], p[:, 3:6], tor, r.bonds, r.rot_idx)
            ymoved = apply_sidechain_torsions(yc, sc.edge_idx, sc.sub, sc.mapping, chi) if self.n_sc else yc
        else:
            moved = modify_conformer_hip(src, p[:, 0:3], p[:, 3:6], tor, r._bonds_i32, r._mask_u8)
            d = mz._sc_dev
            ymoved = apply_sidechain_torsions_hip(yc, d["edge_idx"], d["sub"], d["mapping"], chi) if self.n_sc else yc
        keep = ~fin
        if cyc == 0:
            keep = keep | (torch.arange(rows, device=dev) % R == 0)
        start_x = torch.where(keep[:, None, None], xc, moved).contiguous()
        start_y = torch.where(keep[:, None, None], yc, ymoved).contiguous()
        if starts is not None:
            starts.append((start_x, start_y[:, mov].contiguous()))
        # 2. descent
        step = torch.full((rows,), float(mz.config.step_init), dtype=torch.float64, device=dev)
        zero = torch.zeros(rows, dtype=torch.int32, device=dev)
        xl, yl, _, taken, e_start, el = mz.advance(start_x, start_y, x0r, y0r, step, zero, c.iterations)
        yml = yl[:, mov]
        # 3. Metropolis, 4. best, 5. record
        d = el[:, 5] - st.cur_e[:, 5]
        move = (el[:, 5] < st.cur_e[:, 5]) | (st.u[cyc] < torch.exp(-d / c.temperature))
        improved = el[:, 5] < st.best_e[:, 5]
        st.cur_pos = torch.where(move[:, None, None], xl, xc)
        st.cur_mov = torch.where(move[:, None, None], yml, ymc)
        st.cur_e = torch.where(move[:, None], el, st.cur_e)
        st.best_pos = torch.where(improved[:, None, None], xl, st.best_pos)
        st.best_mov = torch.where(improved[:, None, None], yml, st.best_mov)
        st.best_e = torch.where(improved[:, None], el, st.best_e)
        st.best_cycle = torch.where(improved, torch.full_like(st.best_cycle, cyc), st.best_cycle)
        st.accepted = st.accepted + taken
        st.trace[cyc, :, 0], st.trace[cyc, :, 1] = e_start[:, 5], el[:, 5]
        st.flags[cyc] = move.to(torch.uint8) | (improved.to(torch.uint8) << 1)
        if cyc == 0:
            st.energy_minimized = st.cur_e[::R].clone()

    # ---- results
    def select(self, state: FlexSearchState):
        """(pos [S, n, 3], mov [S, n_mov, 3], energy [S, 6], replica [S], cycle [S]) of the state by the selection rule."""
        return select_flex_torch(state.best_e, state.best_pos, state.best_mov, state.best_cycle, self.config.replicas)

    def result(self, state: FlexSearchState) -> FlexSearchResult:
        """The FlexSearchResult of a state.  A state without a cycle (config.cycles = 0) gives the sampled state back: the identity."""
        mz, R = self.minimizer, self.config.replicas
        x0, y0 = state.x0, state.y0
        S, dev = x0.shape[0], x0.device
        e_before = mz.energy(x0, y0)[0] if S else torch.zeros(0, 6, dtype=torch.float64, device=dev)
        pos, ym, e_after, rep, cyc = self.select(state)
        mov = self._mov.to(dev)
        y = y0.clone()
        y[:, mov] = ym
        e_min = state.energy_minimized
        if state.cycle == 0:
            e_after, e_min = e_before.clone(), e_before.clone()
        q = torch.arange(S, device=dev) * R + rep.long()
        moves = (state.flags[:state.cycle, q] & 1).sum(0).to(torch.int32) if S else torch.zeros(0, dtype=torch.int32, device=dev)
        moved = (pos.double() - x0.double()).pow(2).sum(-1).mean(-1).sqrt().float()
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
