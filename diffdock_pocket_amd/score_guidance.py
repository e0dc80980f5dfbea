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
    the step's device parameter block, params[6]).  A per-step constant: it is NOT multiplied by g^2 dt, exactly as clash guidance,
    so more inference steps mean more total guidance.
 2. Direction.  (d_tr, d_rot, d_tor) = descent.direction_torch(x, g) * w_t, rounded to fp32: exactly what ddp_refine_direction
    writes for step[s] = w_t on this gradient.
 3. Cap factor.  f_s = min(1, max_tr / |d_tr|_2, max_rot / |d_rot|_2, max_tor / max_b |d_tor[b]|), in fp64 from those fp32 values; a
    zero norm contributes no constraint.  The caps are score_guidance_max_tr (Angstrom) and score_guidance_max_rot / _max_tor
    (radians); the defaults 1.0 / 0.5 / 0.5 are untuned choices, fitted to nothing.
 4. Update.  upd_X[s] += (float)(f_s * (double)d_X) for X in tr, rot, tor - added AFTER the SDE / ODE update, after SVGD and after
    clash guidance when that is on too (both may be on, each with its own caps; svgd_only erases neither).  Side-chain updates get no
    guidance.  w_t == 0 writes nothing, not even + 0.
 5. Receptor.  The graph's typed atom nodes, typed as PoseScorer(graph, receptor="graph") types them.  Rigid runs: shared by all
    samples.  Flexible runs: each sample's own current atom_pos, before this step's side-chain update.  The ligand is typed by
    scoring.type_ligand.  Untyped atoms take part in nothing, as in the score.

What the term is not: the score is not validated against smina or Vina; the weight, the schedule and the caps are untuned and the
term is untested on real checkpoints; its torsion component is the heuristic of descent.py (ddp_pose_update re-aligns the conformer
after the torsions, so d_tor is not the exact derivative of the map that is applied, and no accept rule guards it here); it sees
the graph's pocket atoms only, not the full PDB; and the gradient is discontinuous at the ramp ends.  A lower score is not a better
pose.

Two forms of the same arithmetic: `increments_torch`, fp64 PyTorch on host tensors (the CPU `Sampler.step`), and
`ScoreGuidanceWorkspace`, one fused launch of csrc/ddp_score_guidance.hip per step that reads w_t from device memory (the captured
step needs no re-capture when t crosses t_max)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

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

    def launch(self, lig_pos, atom_pos, upd, weight, energy=None, grad=None):
        """lig_pos [S, n, 3]: the poses the scores were computed for; atom_pos: None (the graph's atom nodes, shared) or [S, m, 3]
        (each sample's own atom positions); upd = (tr [S, 3], rot [S, 3], tor [S, T] or None), updated in place; weight: one fp32 value
        in device memory; energy [S, 2] = (inter, intra), grad [S, n, 3] fp64: optional outputs.  All contiguous tensors on the
        workspace's device."""
        from . import launch as LA
        S = lig_pos.shape[0]
        want = [(lig_pos, torch.float32, (S, self.n, 3), "lig_pos"), (upd[0], torch.float32, (S, 3), "upd tr"),
                (upd[1], torch.float32, (S, 3), "upd rot"), (atom_pos, torch.float32, (S, self.m, 3), "atom_pos"),
                (energy, torch.float64, (S, 2), "energy"), (grad, torch.float64, (S, self.n, 3), "grad")]
        if self.T:
            want.append((upd[2], torch.float32, (S, self.T), "upd tor"))
        LA.check_tensors("ScoreGuidanceWorkspace.launch", self.device, want, ("atom_pos", "energy", "grad"), error=ValueError)
        if weight.dtype != torch.float32 or weight.device != self.device or weight.numel() < 1 or not weight.is_contiguous():
            raise ValueError("ScoreGuidanceWorkspace.launch: weight = one fp32 value in device memory")
        a = self.args
        a.n_samples, a.pos, a.weight = S, lig_pos.data_ptr(), weight.data_ptr()
        a.rec, a.rec_stride = (self.rec.data_ptr() or None, 0) if atom_pos is None else (atom_pos.data_ptr() or None, 3 * self.m)
        a.upd[0], a.upd[1], a.upd[2] = upd[0].data_ptr(), upd[1].data_ptr(), (upd[2].data_ptr() if self.T else None)
        a.energy = energy.data_ptr() if energy is not None else None
        a.grad = grad.data_ptr() if grad is not None else None
        LA.score_guidance(a, torch._C._cuda_getCurrentRawStream(lig_pos.device.index))

