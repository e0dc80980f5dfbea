"""The physics-score guidance term of the reverse-diffusion step.  This project's own term - the reference has none.  The clash
guidance of guidance.py steers the sampler away from the receptor and has no attraction; everything attractive the project knows (the
gaussian contact, hydrophobic and hydrogen-bond terms of scoring.py) was applied after sampling only, by the minimisers and the
search, where a pose in the wrong basin stays.  Here every denoising step nudges the poses down the gradient of the Vinardo-form
score itself, along the sampler's own degrees of freedom.  The samples do not interact: sliced samplers, PipelinedSampler, sample
sharding over ranks and flexible receptors all keep working.

Definition.  For sample s at a step with time t, let x be the fp32 pose the scores were computed for and rec the receptor it is held
against, and let g = dE/dx be the fp64 gradient of E(x) = inter(x, rec) + intra(x): the minimiser's energy (minimize.py) at restraint
0, not divided by the torsion factor, with the ScoreConfig form, the typing, the cutoff and the NaN rule of scoring.py.

 1. Per-step weight.  w_t = score_guidance_weight if t <= score_guidance_t_max, else 0 (the weight as the fp32 value that travels in
    the step's device parameter block, slot sampler.P_W_SCORE).  A per-step constant: it is NOT multiplied by g^2 dt, exactly as clash guidance,
    so more inference steps mean more total guidance.
 2. Direction.  (d_tr, d_rot, d_tor) = descent.direction_torch(x, g) * w_t, rounded to fp32: exactly what ddp_refine_direction
    writes for step[s] = w_t on this gradient.
 3. Cap factor.  f_s = min(1, max_tr / |d_tr|_2, max_rot / |d_rot|_2, max_tor / max_b |d_tor[b]|), in fp64 from those fp32 values; a
    zero norm contributes no constraint.  The caps are score_guidance_max_tr (Angstrom) and score_guidance_max_rot / _max_tor
    (radians); the defaults 1.0 / 0.5 / 0.5 are untuned choices, fitted to nothing.
 4. Update.  upd_X[s] += (float)(f_s * (double)d_X) for X in tr, rot, tor - added AFTER the SDE / ODE update, after SVGD and after
    clash guidance when that is on too (both may be on, each with its own caps; svgd_only erases neither).  Side-chain updates get no
    guidance unless score_guidance_sidechains is set (below).  w_t == 0 writes nothing, not even + 0.
 5. Receptor.  The graph's typed atom nodes, typed as PoseScorer(graph, receptor="graph") types them.  Rigid runs: shared by all
    samples.  Flexible runs: each sample's own current atom_pos, before this step's side-chain update.  The ligand is typed by
    scoring.type_ligand.  Untyped atoms take part in nothing, as in the score.

Side chains (SamplerConfig.score_guidance_sidechains, off by default; a flexible run only, otherwise a no-op).  The ligand part above
is unchanged - the ligand increments of a flexible run are exactly what they are without the flag.  For sample s of a flexible run at
a step with w_t > 0 (the same w_t, the same slot), with x as above and y the sample's current atom_pos, before this step's
side-chain update:

 S1. Gradient.  g_y = dE/dy_a over the moving atoms Mv of E(x, y) = inter(x, y) + intra(x) + sc(y): the joint energy of
     minimize_flex.py at both restraints 0, with the tables of minimize_flex.sidechain_tables(graph) (mov, edge_idx, sub, mapping,
     sc_pairs), the receptor typed as PoseScorer(graph, receptor="graph") types it and the same ScoreConfig as the ligand term
     (score_guidance_config).
 S2. Direction.  d_sc = w_t * minimize_flex.direction_sc_torch(y, g_y, ...) in fp64, rounded to fp32.  The sign convention is the
     minimiser's: the angles are applied through the sampler's own side-chain map (apply_sidechain_torsions / ddp_sidechain_update).
 S3. Cap factor.  f_sc = min(1, max_sc / max_j |d_sc[j]|), in fp64 from the fp32 values; a zero maximum gives no constraint.  max_sc
     is score_guidance_max_sc (radians), default 0.5, untuned like the others.  It is a factor of its own, separate from f_s.
 S4. Update.  upd_sc[s, j] += (float)(f_sc * (double)d_sc[j]) - added after the SDE / ODE update and before the side-chain update.
     w_t == 0 writes nothing.

What the side-chain part is not: there is no backbone motion and no rotamer library (a local nudge of the chi angles from where the
sampler has them); the constants are untuned; the score is not validated against smina or Vina; a lower E is not a better pose.  No
restraint term acts inside the step, clash guidance does not reach the side chains, and the receptor is the graph's pocket atoms.

What the term is not: the score is not validated against smina or Vina; the weight, the schedule and the caps are untuned and the
term is untested on real checkpoints; its torsion component is the heuristic of descent.py (ddp_pose_update re-aligns the conformer
after the torsions, so d_tor is not the exact derivative of the map that is applied, and no accept rule guards it here); it sees
the graph's pocket atoms only, not the full PDB; and the gradient is discontinuous at the ramp ends.  A lower score is not a better
pose.

Two forms of the same arithmetic: `increments_torch`, fp64 PyTorch on host tensors (the CPU `Sampler.step`), and
`ScoreGuidanceWorkspace`, one fused launch of csrc/ddp_score_guidance.hip per step that reads w_t from device memory (the captured
step needs no re-capture when t crosses t_max).  The side-chain part likewise: `increments_sc_torch` and
`ScoreGuidanceFlexWorkspace`, one launch of csrc/ddp_score_guidance_flex.hip that REPLACES the ddp_score_guidance launch of the step
and writes the ligand increments (the same bits) and the side-chain increments."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as _L
from .guidance import MAX_ATOMS, MAX_TORSIONS, cap_factor
from .guidance import step_weight  # noqa: F401  (w_t of the definition, the same rule as clash guidance: re-exported)
from .scoring import ScoreConfig


@dataclass
class ScoreGuidanceTables:
    """Host tables of one complex, each from its existing builder: scoring.typed_tables with the graph receptor (every atom node kept,
    a negative radius = untyped), refine.build_self_pairs and descent.ligand_torsions."""
    lig_radii: torch.Tensor        # [n] fp32
    lig_flags: torch.Tensor        # [n] uint8
    rec: torch.Tensor              # [m, 3] fp32: the graph's atom nodes
    rec_radii: torch.Tensor        # [m] fp32
    rec_flags: torch.Tensor        # [m] uint8
    self_pairs: torch.Tensor       # [n, n] uint8, upper triangle (None: no ligand-ligand term)
    bonds: torch.Tensor            # [T, 2] int64 (u, v)
    mask_rotate: torch.Tensor      # [T, n] bool
    config: ScoreConfig

    @property
    def n(self) -> int:
        return int(self.lig_radii.shape[0])


def build_tables(graph, torsions: bool = True, config: Optional[ScoreConfig] = None) -> ScoreGuidanceTables:
    """The tables of a complex graph.  torsions=False (SamplerConfig.no_torsion): no rotatable bond takes part, the direction is
    rigid only.  config: the constants of the form (None: ScoreConfig()).  Raises above the kernel's limits, whatever device the
    sampler runs on."""
    from .descent import ligand_torsions
    from .refine import build_self_pairs
    from .scoring import typed_tables
    config = (config or ScoreConfig()).check()
    t, _ = typed_tables(graph, "graph")
    n = int(t["lig_r"].shape[0])
    bonds, mask = ligand_torsions(graph)
    pairs = build_self_pairs(n, torch.as_tensor(graph["ligand", "ligand"].edge_index).numpy(), mask.numpy())
    if not torsions:
        bonds, mask = bonds[:0], mask[:0]
    if n > MAX_ATOMS or bonds.shape[0] > MAX_TORSIONS:
        raise ValueError(f"score guidance: a ligand of {n} atoms and {bonds.shape[0]} rotatable bonds exceeds the limits of "
                         f"ddp_score_guidance ({MAX_ATOMS} atoms, {MAX_TORSIONS} bonds)")
    return ScoreGuidanceTables(t["lig_r"].float().contiguous(), t["lig_f"].to(torch.uint8).contiguous(), t["rec"].float().contiguous(),
                               t["rec_r"].float().contiguous(), t["rec_f"].to(torch.uint8).contiguous(), pairs.contiguous(), bonds,
                               mask.bool(), config)


def increments_torch(x, rec, tables: ScoreGuidanceTables, w_t: float, caps):
    """(inc_tr [S, 3], inc_rot [S, 3], inc_tor [S, T]) fp32: the increments of step 4 for host poses x [S, n, 3] fp32 against rec
    [m, 3] (shared) or [S, m, 3] (each sample's own atom_pos), caps = (max_tr, max_rot, max_tor); None when w_t is not above 0
    (nothing is to be added)."""
    from .descent import direction_torch
    from .minimize import energy_torch
    if not w_t > 0:
        return None
    x = x.float()
    _, g = energy_torch(x, x, tables.lig_radii, tables.lig_flags, rec.float(), tables.rec_radii, tables.rec_flags, tables.self_pairs,
                        tables.config, 0.0)
    d = [(w_t * v).float() for v in direction_torch(x, g, tables.bonds, tables.mask_rotate)]
    f = cap_factor(d[0], d[1], d[2], *caps)
    return tuple((f[:, None] * v.double()).float() for v in d)


# the limits of ddp_score_guidance_flex, the header's values
FLEX_MAX_ATOMS, FLEX_MAX_TORSIONS = _L.DDP_SCORE_GUIDANCE_FLEX_MAX_ATOMS, _L.DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS
FLEX_MAX_MOVING, FLEX_MAX_BONDS = _L.DDP_SCORE_GUIDANCE_FLEX_MAX_MOVING, _L.DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS


def check_flex_limits(who: str, n: int, T: int, n_mov: int, n_sc: int):
    """Raises above the limits of ddp_score_guidance_flex, whatever device the sampler runs on."""
    if n > FLEX_MAX_ATOMS or T > FLEX_MAX_TORSIONS or n_mov > FLEX_MAX_MOVING or n_sc > FLEX_MAX_BONDS:
        raise ValueError(f"{who}: {n} ligand atoms, {T} rotatable bonds, {n_mov} moving atoms and {n_sc} side-chain bonds exceed the "
                         f"limits of ddp_score_guidance_flex ({FLEX_MAX_ATOMS} atoms, {FLEX_MAX_TORSIONS} bonds, {FLEX_MAX_MOVING} moving "
                         f"atoms, {FLEX_MAX_BONDS} side-chain bonds)")


def build_sidechain_tables(graph, tables: ScoreGuidanceTables):
    """The side-chain tables of the term for a complex graph with flexResidues: minimize_flex.sidechain_tables (checked on the host by
    check_sidechain_tables), None for a graph without them.  tables: the ligand term's, of the same graph.  Raises above the limits of
    ddp_score_guidance_flex, whatever device the sampler runs on."""
    from .minimize_flex import sidechain_tables
    sc = sidechain_tables(graph)
    if sc is None:
        return None
    check_flex_limits("score guidance of side chains", tables.n, int(tables.bonds.shape[0]), sc.n_mov, sc.n_sc)
    return sc


def cap_factor_sc(d_sc, max_sc):
    """f_sc [S] fp64 of step S3 from the fp32 direction d_sc [S, n_sc]."""
    f = torch.ones(d_sc.shape[0], dtype=torch.float64)
    if d_sc.shape[1] == 0:
        return f
    mx = d_sc.double().abs().max(-1)[0]
    return torch.where(mx > 0, torch.minimum(f, float(max_sc) / mx.clamp(min=1e-300)), f)


def increments_sc_torch(x, y, tables: ScoreGuidanceTables, sc_tables, w_t: float, max_sc: float):
    """inc_sc [S, n_sc] fp32: the increments of step S4 for host poses x [S, n, 3] fp32 and each sample's own receptor atoms y
    [S, m, 3] fp32; sc_tables: a minimize_flex.SidechainTables; None when w_t is not above 0 (nothing is to be added)."""
    from .minimize_flex import direction_sc_torch, energy_flex_torch
    if not w_t > 0:
        return None
    x, y, sc = x.float(), y.float(), sc_tables
    _, _, gy = energy_flex_torch(x, y, x, y, tables.lig_radii, tables.lig_flags, tables.rec_radii, tables.rec_flags, tables.self_pairs,
                                 sc.mov, sc.pairs, tables.config, 0.0, 0.0)
    d = (w_t * direction_sc_torch(y, gy, sc.mov, sc.edge_idx, sc.sub, sc.mapping)).float()
    return (cap_factor_sc(d, max_sc)[:, None] * d.double()).float()


class ScoreGuidanceWorkspace:
    """Device side: the tables uploaded once and the argument struct of ddp_score_guidance; `launch` enqueues the one launch on the
    current stream (no host work besides it: capturable)."""

    def __init__(self, tables: ScoreGuidanceTables, device, caps=(1.0, 0.5, 0.5)):
        from . import _lib as L
        from . import launch as LA
        self.tables = tables
        self.n, self.T, self.m = tables.n, int(tables.bonds.shape[0]), int(tables.rec_radii.shape[0])
        self.lig_radii, self.rec, self.rec_radii = (t.float().contiguous().to(device) for t in (tables.lig_radii, tables.rec, tables.rec_radii))
        self.lig_flags, self.rec_flags = (t.to(torch.uint8).contiguous().to(device) for t in (tables.lig_flags, tables.rec_flags))
        self.self_pairs = tables.self_pairs.to(torch.uint8).contiguous().to(device) if tables.self_pairs is not None else None
        self.device = self.lig_radii.device                  # (with its index, as the tensors of `launch` carry it)
        self.bonds = LA.refine_bonds(tables.bonds, self.n, device) if self.T else None       # checked on the host, uploaded once
        self.mask_rotate = tables.mask_rotate.to(torch.uint8).contiguous().to(device) if self.T else None
        a = self.args = L.ScoreGuidanceArgs(n=self.n, m=self.m, n_tor=self.T, form=L.ScoreForm.from_config(tables.config),
                                            max_tr=float(caps[0]), max_rot=float(caps[1]), max_tor=float(caps[2]))
        a.lig_radii, a.lig_flags = self.lig_radii.data_ptr(), self.lig_flags.data_ptr()
        a.rec_radii, a.rec_flags = self.rec_radii.data_ptr() or None, self.rec_flags.data_ptr() or None
        a.self_pairs = self.self_pairs.data_ptr() if self.self_pairs is not None else None
        a.bonds = self.bonds.data_ptr() if self.T else None
        a.mask_rotate = self.mask_rotate.data_ptr() if self.T else None

    def _bind(self, who, a, lig_pos, atom_pos, upd, weight, energy, width, more, optional):
        """Checks the tensors of a launch and binds what both argument structs hold: n_samples, pos, weight, rec, rec_stride,
        upd[0 .. 2] and energy [S, width].  more: the caller's own (tensor, dtype, shape, name) entries for a given S; optional: the
        names that may be None."""
        from . import launch as LA
        S = lig_pos.shape[0]
        want = [(lig_pos, torch.float32, (S, self.n, 3), "lig_pos"), (upd[0], torch.float32, (S, 3), "upd tr"),
                (upd[1], torch.float32, (S, 3), "upd rot"), (atom_pos, torch.float32, (S, self.m, 3), "atom_pos"),
                (energy, torch.float64, (S, width), "energy")] + more(S)
        if self.T:
            want.append((upd[2], torch.float32, (S, self.T), "upd tor"))
        LA.check_tensors(who, self.device, want, optional, error=ValueError)
        if weight.dtype != torch.float32 or weight.device != self.device or weight.numel() < 1 or not weight.is_contiguous():
            raise ValueError(f"{who}: weight = one fp32 value in device memory")
        a.n_samples, a.pos, a.weight = S, lig_pos.data_ptr(), weight.data_ptr()
        a.rec, a.rec_stride = (self.rec.data_ptr() or None, 0) if atom_pos is None else (atom_pos.data_ptr() or None, 3 * self.m)
        a.upd[0], a.upd[1], a.upd[2] = upd[0].data_ptr(), upd[1].data_ptr(), (upd[2].data_ptr() if self.T else None)
        a.energy = energy.data_ptr() if energy is not None else None
        return torch._C._cuda_getCurrentRawStream(lig_pos.device.index)

    def launch(self, lig_pos, atom_pos, upd, weight, energy=None, grad=None):
        """lig_pos [S, n, 3]: the poses the scores were computed for; atom_pos: None (the graph's atom nodes, shared) or [S, m, 3]
        (each sample's own atom positions); upd = (tr [S, 3], rot [S, 3], tor [S, T] or None), updated in place; weight: one fp32 value
        in device memory; energy [S, 2] = (inter, intra), grad [S, n, 3] fp64: optional outputs.  All contiguous tensors on the
        workspace's device."""
        from . import launch as LA
        a = self.args
        st = self._bind("ScoreGuidanceWorkspace.launch", a, lig_pos, atom_pos, upd, weight, energy, 2,
                        lambda S: [(grad, torch.float64, (S, self.n, 3), "grad")], ("atom_pos", "energy", "grad"))
        a.grad = grad.data_ptr() if grad is not None else None
        LA.score_guidance(a, st)


class ScoreGuidanceFlexWorkspace(ScoreGuidanceWorkspace):
    """Device side of the term with the side chains guided: the ligand tables of ScoreGuidanceWorkspace, the side-chain tables
    (launch.flex_tables: checked on the host, uploaded once) and the argument struct of ddp_score_guidance_flex; `launch` enqueues the
    one launch on the current stream (no host work besides it: capturable)."""

    def __init__(self, tables: ScoreGuidanceTables, sc_tables, device, caps=(1.0, 0.5, 0.5), max_sc: float = 0.5):
        from . import _lib as L
        from . import launch as LA
        super().__init__(tables, device, caps)
        self.sc_tables = sc_tables
        self.n_mov, self.n_sc, self.n_sub = sc_tables.n_mov, sc_tables.n_sc, int(sc_tables.sub.shape[0])
        check_flex_limits("ScoreGuidanceFlexWorkspace", self.n, self.T, self.n_mov, self.n_sc)
        self._sc_dev = LA.flex_tables(sc_tables, self.m, device)
        b, d = self.args, self._sc_dev
        a = self.flex_args = L.ScoreGuidanceFlexArgs(n=self.n, m=self.m, n_tor=self.T, form=b.form, max_tr=b.max_tr, max_rot=b.max_rot,
                                                     max_tor=b.max_tor, n_mov=self.n_mov, n_sc=self.n_sc, n_sub=self.n_sub,
                                                     max_sc=float(max_sc))
        for k in ("lig_radii", "lig_flags", "rec_radii", "rec_flags", "self_pairs", "bonds", "mask_rotate"):
            setattr(a, k, getattr(b, k))
        a.mov, a.sc_edge_idx, a.sc_sub = (d[k].data_ptr() or None for k in ("mov", "edge_idx", "sub"))
        a.sc_map, a.sc_pairs = d["mapping"].data_ptr() or None, d["pairs"].data_ptr() or None

    def launch(self, lig_pos, atom_pos, upd, weight, upd_sc, energy=None, grad_mov=None):
        """lig_pos, upd, weight as ScoreGuidanceWorkspace.launch; atom_pos [S, m, 3]: each sample's own atom positions (only read);
        upd_sc [S, n_sc] fp32, updated in place (None with n_sc = 0); energy [S, 3] = (inter, intra, sc), grad_mov [S, n_mov, 3] fp64:
        optional outputs.  All contiguous tensors on the workspace's device."""
        from . import launch as LA
        a = self.flex_args
        more = lambda S: [(grad_mov, torch.float64, (S, self.n_mov, 3), "grad_mov")] + \
            ([(upd_sc, torch.float32, (S, self.n_sc), "upd sc")] if self.n_sc else [])
        st = self._bind("ScoreGuidanceFlexWorkspace.launch", a, lig_pos, atom_pos, upd, weight, energy, 3, more, ("energy", "grad_mov"))
        a.upd_sc = upd_sc.data_ptr() if self.n_sc else None
        a.grad_mov = grad_mov.data_ptr() if grad_mov is not None else None
        LA.score_guidance_flex(a, st)
