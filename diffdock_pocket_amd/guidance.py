"""The steric-clash guidance term of the reverse-diffusion step.  This project's own term - the reference has none: its sampler knows
the receptor's van der Waals surface only through what the score model learned, and the clash relief (refine.py), the physics score
and the minimisers repair the poses after sampling.  Here every denoising step nudges the poses down the gradient of the clash energy
of refine.py, along the sampler's own degrees of freedom.  Unlike SVGD the samples do not interact: sliced samplers, PipelinedSampler,
sample sharding over ranks and flexible receptors all keep working.

Definition.  For sample s at a step with time t, let x be the fp32 pose the scores were computed for and rec the receptor it is held
against, and let g = dE/dx be the fp64 gradient of E = E_cross + E_self of refine.py with restraint 0, the evaluator's radii
(assets/vdw_radii.json), overlap = OVERLAP_DISTANCE and receptor hydrogens ignored.

 1. Per-step weight.  w_t = clash_guidance_weight if t <= clash_guidance_t_max, else 0 (the weight as the fp32 value that travels in
    the step's device parameter block, slot sampler.P_W_CLASH).  A per-step constant: it is NOT multiplied by g^2 dt, so more
    inference steps mean more total guidance.
 2. Direction.  (d_tr, d_rot, d_tor) = descent.direction_torch(x, g) * w_t, rounded to fp32: exactly what ddp_refine_direction
    writes for step[s] = w_t.
 3. Cap factor.  f_s = min(1, max_tr / |d_tr|_2, max_rot / |d_rot|_2, max_tor / max_b |d_tor[b]|), in fp64 from those fp32 values; a
    zero norm contributes no constraint.  The caps are clash_guidance_max_tr (Angstrom) and clash_guidance_max_rot / _max_tor
    (radians); the defaults 1.0 / 0.5 / 0.5 are untuned choices, fitted to nothing.
 4. Update.  upd_X[s] += (float)(f_s * (double)d_X) for X in tr, rot, tor - added AFTER the SDE / ODE update and after SVGD (svgd_only
    does not erase it).  Side-chain updates get no guidance.  w_t == 0 writes nothing, not even + 0.
 5. Receptor.  Rigid runs: the graph's atom nodes, shared by all samples.  Flexible runs: each sample's own current atom_pos, before
    this step's side-chain update.  A full-PDB receptor is out of scope.

What the term is not: it has no attraction (it can only push atoms apart), its schedule and caps are untuned, its torsion component is
a heuristic (ddp_pose_update re-aligns the conformer after the torsions, so d_tor is not the exact derivative of the map that is
applied, and no accept rule guards it here), and it has not been validated on real checkpoints.

Two forms of the same arithmetic: `increments_torch`, fp64 PyTorch on host tensors (the CPU `Sampler.step`), and `GuidanceWorkspace`,
one fused launch of csrc/ddp_guidance.hip per step that reads w_t from device memory (the captured step needs no re-capture)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from .evaluation import OVERLAP_DISTANCE, PoseEvaluator

MAX_ATOMS, MAX_TORSIONS = 1024, 1024      # DDP_EVAL_MAX_ATOMS, DDP_GUIDANCE_MAX_TORSIONS of include/ddp_hip.h


@dataclass
class GuidanceTables:
    """Host tables of one complex, each from its existing builder: the van der Waals radii of PoseEvaluator (a negative receptor
    radius = a hydrogen), the graph's atom nodes, refine.build_self_pairs and descent.ligand_torsions."""
    lig_radii: torch.Tensor        # [n] fp32
    rec: torch.Tensor              # [m, 3] fp32: the graph's atom nodes
    rec_radii: torch.Tensor        # [m] fp32
    self_pairs: torch.Tensor       # [n, n] uint8, upper triangle (None: no ligand-ligand term)
    bonds: torch.Tensor            # [T, 2] int64 (u, v)
    mask_rotate: torch.Tensor      # [T, n] bool

    @property
    def n(self) -> int:
        return int(self.lig_radii.shape[0])


def build_tables(graph, torsions: bool = True) -> GuidanceTables:
    """The tables of a complex graph.  torsions=False (SamplerConfig.no_torsion): no rotatable bond takes part, the direction is
    rigid only.  Raises above the kernel's limits, whatever device the sampler runs on."""
    from .descent import ligand_torsions
    from .refine import build_self_pairs
    ev = PoseEvaluator(graph, "cpu", receptor="graph", max_automorphisms=1)
    lig_r, rec, rec_r = ev.contact_tables(False)
    bonds, mask = ligand_torsions(graph)
    pairs = build_self_pairs(ev.n, torch.as_tensor(graph["ligand", "ligand"].edge_index).numpy(), mask.numpy())
    if not torsions:
        bonds, mask = bonds[:0], mask[:0]
    if ev.n > MAX_ATOMS or bonds.shape[0] > MAX_TORSIONS:
        raise ValueError(f"clash guidance: a ligand of {ev.n} atoms and {bonds.shape[0]} rotatable bonds exceeds the limits of "
                         f"ddp_clash_guidance ({MAX_ATOMS} atoms, {MAX_TORSIONS} bonds)")
    return GuidanceTables(lig_r.contiguous(), rec.contiguous(), rec_r.contiguous(), pairs.contiguous(), bonds, mask.bool())


def step_weight(weight: float, t: float, t_max: float) -> float:
    """w_t of the definition, as the fp32 value the device reads."""
    return float(torch.tensor(weight if t <= t_max else 0.0, dtype=torch.float32))


def cap_factor(d_tr, d_rot, d_tor, max_tr, max_rot, max_tor):
    """f_s [S] fp64 from the fp32 direction (d_tor [S, T] or None)."""
    f = torch.ones(d_tr.shape[0], dtype=torch.float64)
    norms = [(d_tr.double().pow(2).sum(-1).sqrt(), max_tr), (d_rot.double().pow(2).sum(-1).sqrt(), max_rot)]
    if d_tor is not None and d_tor.shape[1] > 0:
        norms.append((d_tor.double().abs().max(-1)[0], max_tor))
    for nrm, cap in norms:
        f = torch.where(nrm > 0, torch.minimum(f, float(cap) / nrm.clamp(min=1e-300)), f)
    return f


def increments_torch(x, rec, tables: GuidanceTables, w_t: float, max_tr: float, max_rot: float, max_tor: float,
                     overlap: float = OVERLAP_DISTANCE):
    """(inc_tr [S, 3], inc_rot [S, 3], inc_tor [S, T]) fp32: the increments of step 4 for host poses x [S, n, 3] fp32 against rec
    [m, 3] (shared) or [S, m, 3] (each sample's own atom_pos); None when w_t is not above 0 (nothing is to be added)."""
    from .descent import direction_torch
    from .refine import energy_torch
    if not w_t > 0:
        return None
    x = x.float()
    _, g = energy_torch(x, x, tables.lig_radii, rec.float(), tables.rec_radii, tables.self_pairs, overlap, 0.0)
    d = [(w_t * v).float() for v in direction_torch(x, g, tables.bonds, tables.mask_rotate)]
    f = cap_factor(d[0], d[1], d[2], max_tr, max_rot, max_tor)
    return tuple((f[:, None] * v.double()).float() for v in d)


class GuidanceWorkspace:
    """Device side: the tables uploaded once and the argument struct of ddp_clash_guidance; `launch` enqueues the one launch on the
    current stream (no host work besides it: capturable)."""

    def __init__(self, tables: GuidanceTables, device, max_tr=1.0, max_rot=0.5, max_tor=0.5, overlap: float = OVERLAP_DISTANCE):
        from . import _lib as L
        from . import launch as LA
        self.tables, self.device = tables, torch.device(device)
        self.n, self.T, self.m = tables.n, int(tables.bonds.shape[0]), int(tables.rec_radii.shape[0])
        self.lig_radii, self.rec, self.rec_radii = (t.float().contiguous().to(device) for t in (tables.lig_radii, tables.rec, tables.rec_radii))
        self.self_pairs = tables.self_pairs.to(torch.uint8).contiguous().to(device) if tables.self_pairs is not None else None
        self.device = self.lig_radii.device                  # (with its index, as the tensors of `launch` carry it)
        self.bonds = LA.refine_bonds(tables.bonds, self.n, device) if self.T else None       # checked on the host, uploaded once
        self.mask_rotate = tables.mask_rotate.to(torch.uint8).contiguous().to(device) if self.T else None
        a = self.args = L.GuidanceArgs(n=self.n, m=self.m, n_tor=self.T, overlap=float(overlap), max_tr=float(max_tr),
                                       max_rot=float(max_rot), max_tor=float(max_tor))
        a.lig_radii, a.rec_radii = self.lig_radii.data_ptr(), self.rec_radii.data_ptr() or None
        a.self_pairs = self.self_pairs.data_ptr() if self.self_pairs is not None else None
        a.bonds = self.bonds.data_ptr() if self.T else None
        a.mask_rotate = self.mask_rotate.data_ptr() if self.T else None

    def launch(self, pos, rec, upd, weight, energy=None, grad=None):
        """pos [S, n, 3]: the poses the scores were computed for; rec: None (the graph's atom nodes, shared) or [S, m, 3] (each
        sample's own atom positions); upd = (tr [S, 3], rot [S, 3], tor [S, T] or None), updated in place; weight: one fp32 value in
        device memory; energy [S, 2], grad [S, n, 3] fp64: optional outputs.  All contiguous tensors on the workspace's device."""
        from . import launch as LA
        S = pos.shape[0]
        want = [(pos, torch.float32, (S, self.n, 3), "pos"), (upd[0], torch.float32, (S, 3), "upd tr"), (upd[1], torch.float32, (S, 3), "upd rot"),
                (rec, torch.float32, (S, self.m, 3), "rec"), (energy, torch.float64, (S, 2), "energy"), (grad, torch.float64, (S, self.n, 3), "grad")]
        if self.T:
            want.append((upd[2], torch.float32, (S, self.T), "upd tor"))
        LA.check_tensors("GuidanceWorkspace.launch", self.device, want, ("rec", "energy", "grad"), error=ValueError)
        if weight.dtype != torch.float32 or weight.device != self.device or weight.numel() < 1 or not weight.is_contiguous():
            raise ValueError("GuidanceWorkspace.launch: weight = one fp32 value in device memory")
        a = self.args
        a.n_samples, a.pos, a.weight = S, pos.data_ptr(), weight.data_ptr()
        a.rec, a.rec_stride = (self.rec.data_ptr() or None, 0) if rec is None else (rec.data_ptr() or None, 3 * self.m)
        a.upd[0], a.upd[1], a.upd[2] = upd[0].data_ptr(), upd[1].data_ptr(), (upd[2].data_ptr() if self.T else None)
        a.energy = energy.data_ptr() if energy is not None else None
        a.grad = grad.data_ptr() if grad is not None else None
        LA.clash_guidance(a, torch._C._cuda_getCurrentRawStream(pos.device.index))


def check_config(weight, t_max, max_tr, max_rot, max_tor, prefix: str = "clash_guidance"):
    """Negative or NaN values raise (a cap of +infinity is allowed: no cap).  prefix: the SamplerConfig fields' common name, for the
    messages (score_guidance.py checks its own five through here)."""
    for name, v in (("weight", weight), ("t_max", t_max), ("max_tr", max_tr), ("max_rot", max_rot), ("max_tor", max_tor)):
        if not float(v) >= 0.0:
            raise ValueError(f"{prefix}_{name} must not be negative or NaN, got {v!r}")
    if math.isinf(float(weight)):
        raise ValueError(f"{prefix}_weight must be finite")
