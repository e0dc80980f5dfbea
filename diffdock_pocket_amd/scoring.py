"""A Vinardo-form empirical score of sampled poses: the functional form and the constants of Vinardo (Quiroga & Villarreal, PLoS ONE
2016) with Vina's X-Score-style atom typing, over ligand-receptor heavy-atom pairs.  Neither smina nor Vina was at hand when this was
written: the score is NOT validated against either, the constants are as published and untuned here, and no number it gives should
be read as a smina or Vina number.  It ranks poses when there is no confidence model and says whether a pose makes physical sense
beyond a clash count; it does not replace the confidence model.

Atom types.  Every atom gets a radius (fp32) and a flag byte: bit 0 hydrophobic, bit 1 hydrogen-bond donor, bit 2 acceptor.  Radii in
angstrom (assets/vinardo_types.json): C 2.0, N 1.75, O 1.6, P 2.1, S 2.0, F 1.545, Cl 2.045, Br 2.165, I 2.36.  Hydrogens and every
other element (metals, B, Si, Se, ...) get radius -1 ("untyped") and take part in nothing.
    C           hydrophobic iff every bonded heavy neighbour is C
    F Cl Br I   hydrophobic
    S P         no flags
    O           always an acceptor; a donor iff it carries a hydrogen
    N           a donor iff it carries a hydrogen; acceptor: see below
  Ligand, from the graph alone: element, hydrogen count, formal charge and hybridisation are ligand.x columns 0, 5, 3, 7, heavy
  neighbours come from ("ligand", "ligand").edge_index.  N is an acceptor iff it has no hydrogen, formal charge <= 0, and either at most
  2 heavy neighbours or hybridisation SP3 (inputs.perceive already turns amide- and aniline-like N into SP2).
  Receptor: bonds follow a distance rule over the typed atoms, bonded iff d < 1.1 (cov_i + cov_j) with the covalent radii C 0.77,
  N 0.75, O 0.73, P 1.06, S 1.02, F 0.71, Cl 0.99, Br 1.14, I 1.33.  "Carries a hydrogen" is decided by residue and atom name, not by
  H records: backbone N of every residue but PRO; ARG NE NH1 NH2; ASN ND2; GLN NE2; HIS ND1 NE2; LYS NZ; TRP NE1; SER OG; THR OG1;
  TYR OH.  HIP / HIE / HID / HIZ count as HIS, the phospho- and variant residues of inputs.AMINO_ACIDS as their parent residue where the
  atom name exists.  Receptor N is an acceptor only for HIS ND1 / NE2.  In a residue the table does not know: N is a donor and not an
  acceptor, O is both.
  Two receptor sources give identical types for the same atoms: the graph's atom nodes (atom.x columns 0, 1, 3: residue, element,
  atom name) and PDB text shifted by original_center (`typed_receptor`, the counterpart of PoseEvaluator.full_receptor with the names
  kept; the names go through the same vocabularies as the graph's).

Pair terms, over ligand atom i and receptor atom j, both typed, with centre distance d < 8 A (strict); s = d - R_i - R_j:
    gauss       = exp(-(s / 0.8)^2)
    repulsion   = s^2 if s < 0, else 0
    hydrophobic = (both atoms hydrophobic)              1 for s <= 0, linear to 0 at s = 2.5
    hbond       = (a donor-acceptor pair, either way)   1 for s <= -0.6, linear to 0 at s = 0
Sums and totals:
    inter = -0.045 sum gauss + 0.8 sum repulsion - 0.035 sum hydrophobic - 0.6 sum hbond
    intra = the same weighted sum over the ligand pairs of refine.build_self_pairs (more than 3 bonds apart AND separated by a
            rotatable bond); reported, NOT part of total
    total = inter / (1 + 0.0585 N_tor),  N_tor = the rows of sampler.torsion_tables(graph)
Gradient (optional): grad_i = d(inter + intra)/dx_i, not scaled by the torsion divisor.  The linear terms have their slope on the open
intervals only and 0 at and outside the kinks; a pair with d = 0 adds its energy and no gradient.
All arithmetic is fp64 on the fp32 inputs (converted first).  A NaN coordinate gives NaN for that sample only.

What the score is not: validated against smina or Vina; directional in its hydrogen bonds (a donor-acceptor pair counts whatever the
angle); a desolvation or electrostatic model; aware of metals or of explicit hydrogens.

Device tensors go through csrc/ddp_score.hip (ddp_pose_score: one workgroup per sample, one launch); CPU tensors through the
PyTorch fp64 form below (`score_torch`), chunked over the samples."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .inputs import AMINO_ACIDS, ATOM_TYPE_3, ATOMIC_NUMBER, ATOMIC_NUMS, FORMAL_CHARGE, HYBRIDIZATION, NUM_H, parse_pdb, safe_index
from .pose_args import check_poses
from .refine import build_self_pairs, ligand_torsions

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
HYDROPHOBIC, DONOR, ACCEPTOR = 1, 2, 4


def _load_tables():
    with open(os.path.join(ASSETS, "vinardo_types.json")) as f:
        return json.load(f)


TABLES = _load_tables()
RADII = {ATOMIC_NUMBER[k]: float(v) for k, v in TABLES["radii"].items()}                  # atomic number -> Vinardo radius
COVALENT = {ATOMIC_NUMBER[k]: float(v) for k, v in TABLES["covalent_radii"].items()}
_HALOGENS = (9, 17, 35, 53)


@dataclass
class ScoreConfig:
    """The constants of the form, as published for Vinardo; untuned here.  The weights carry their signs."""
    cutoff: float = 8.0
    gauss_offset: float = 0.0
    gauss_width: float = 0.8
    hydrophobic_good: float = 0.0
    hydrophobic_bad: float = 2.5
    hbond_good: float = -0.6
    hbond_bad: float = 0.0
    w_gauss: float = -0.045
    w_repulsion: float = 0.8
    w_hydrophobic: float = -0.035
    w_hbond: float = -0.6
    w_torsion: float = 0.0585      # total = inter / (1 + w_torsion N_tor)

    def check(self):
        if not (self.cutoff > 0 and np.isfinite(self.cutoff)):
            raise ValueError("ScoreConfig: cutoff must be positive and finite")
        if not (self.gauss_width > 0 and self.hydrophobic_bad > self.hydrophobic_good and self.hbond_bad > self.hbond_good):
            raise ValueError("ScoreConfig: gauss_width must be positive and every ramp must have good < bad")
        if not self.w_torsion >= 0:
            raise ValueError("ScoreConfig: w_torsion must not be negative")
        return self


@dataclass
class PoseScores:
    """Per-sample scores of PoseScorer.score, in the order of the poses handed in, on their device; fp64."""
    terms: torch.Tensor                    # [S, 4] unweighted sums over the ligand-receptor pairs: gauss, repulsion, hydrophobic, hbond
    inter: torch.Tensor                    # [S]
    intra: torch.Tensor                    # [S] (not part of total)
    total: torch.Tensor                    # [S] inter / (1 + w_torsion N_tor): lower is better
    grad: Optional[torch.Tensor] = None    # [S, n, 3] d(inter + intra)/dx, with_grad only

    def _map(self, fn) -> "PoseScores":
        return PoseScores(**{k: (None if v is None else fn(v)) for k, v in self.__dict__.items()})

    def cpu(self) -> "PoseScores":
        return self._map(lambda t: t.cpu())

    def index(self, order) -> "PoseScores":
        return self._map(lambda t: t[order.to(t.device)])


@dataclass
class TypedReceptor:
    """A receptor with its types, in a graph's frame: what `typed_receptor` returns and PoseScorer(receptor=...) takes."""
    coords: np.ndarray      # [m, 3] float32
    radii: np.ndarray       # [m] float32, -1: untyped
    flags: np.ndarray       # [m] uint8


# ---------------------------------------------------------------------------------------------- typing
def _radii_of(z: np.ndarray) -> np.ndarray:
    return np.array([RADII.get(int(v), -1.0) for v in z], dtype=np.float32)


def ligand_types(z: Sequence[int], num_h: Sequence[int], formal_charge: Sequence[int], hybridization: Sequence[str], edge_index):
    """(radii [n] float32, flags [n] uint8) of ligand atoms: atomic numbers, hydrogen counts, formal charges, hybridisation names
    ("SP", "SP2", "SP3", ...) and the bond list [2, E] (either or both directions).  A bonded explicit hydrogen counts as a carried
    hydrogen and never as a heavy neighbour."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    n = len(z)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    nbrs = [set() for _ in range(n)]
    for a, b in ei.T.tolist():
        if a != b and 0 <= a < n and 0 <= b < n:
            nbrs[a].add(b)
            nbrs[b].add(a)
    radii = _radii_of(z)
    flags = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        if radii[i] < 0:
            continue
        heavy = [j for j in nbrs[i] if z[j] != 1]
        has_h = int(num_h[i]) > 0 or any(z[j] == 1 for j in nbrs[i])
        zi, f = int(z[i]), 0
        if zi == 6:
            f = HYDROPHOBIC if all(z[j] == 6 for j in heavy) else 0
        elif zi in _HALOGENS:
            f = HYDROPHOBIC
        elif zi == 8:
            f = ACCEPTOR | (DONOR if has_h else 0)
        elif zi == 7:
            f = DONOR if has_h else 0
            if not has_h and int(formal_charge[i]) <= 0 and (len(heavy) <= 2 or str(hybridization[i]).upper() == "SP3"):
                f |= ACCEPTOR
        flags[i] = f
    return radii, flags


def type_ligand(graph):
    """(radii, flags) of a complex graph's ligand nodes (see the module docstring)."""
    x = torch.as_tensor(graph["ligand"].x).long().numpy()
    z = [ATOMIC_NUMS[i] if ATOMIC_NUMS[i] != "misc" else 0 for i in x[:, 0].tolist()]
    num_h = [NUM_H[i] if NUM_H[i] != "misc" else 9 for i in x[:, 5].tolist()]
    charge = [FORMAL_CHARGE[i] if FORMAL_CHARGE[i] != "misc" else 0 for i in x[:, 3].tolist()]
    hyb = [HYBRIDIZATION[i] for i in x[:, 7].tolist()]
    return ligand_types(z, num_h, charge, hyb, torch.as_tensor(graph["ligand", "ligand"].edge_index).numpy())


def distance_bonds(coords: np.ndarray, z: np.ndarray) -> list:
    """Neighbour lists of the distance rule over the typed atoms: i ~ j iff d_ij < bond_tolerance (cov_i + cov_j), fp64."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    cov = np.array([COVALENT.get(int(v), -1.0) for v in z], dtype=np.float64)
    typed = np.nonzero(cov > 0)[0]
    nbrs = [[] for _ in range(len(z))]
    tol = float(TABLES["bond_tolerance"])
    xt, ct = coords[typed], cov[typed]
    for a0 in range(0, len(typed), 512):
        d = np.linalg.norm(xt[a0:a0 + 512, None, :] - xt[None, :, :], axis=-1)
        hit = d < tol * (ct[a0:a0 + 512, None] + ct[None, :])
        for a, b in zip(*np.nonzero(hit)):
            if a0 + a != b:
                nbrs[int(typed[a0 + a])].append(int(typed[b]))
    return nbrs


def receptor_types(res_index: Sequence[int], z: Sequence[int], name_index: Sequence[int], coords):
    """(radii [m] float32, flags [m] uint8) of receptor atoms given as the graph gives them: index into inputs.AMINO_ACIDS, atomic number,
    index into inputs.ATOM_TYPE_3 (the last entry of either vocabulary: not known), and the coordinates the bonds are perceived on."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    m = len(z)
    radii = _radii_of(z)
    flags = np.zeros(m, dtype=np.uint8)
    nbrs = distance_bonds(coords, z)
    known, parents, donors = set(TABLES["residues"]), TABLES["parents"], TABLES["donors"]
    for i in range(m):
        if radii[i] < 0:
            continue
        res = AMINO_ACIDS[int(res_index[i])]
        res = parents.get(res, res)
        name = ATOM_TYPE_3[int(name_index[i])]
        zi, f = int(z[i]), 0
        if res in known:
            has_h = name in donors.get(res, ()) or (name == TABLES["backbone_donor"] and res not in TABLES["no_backbone_donor"])
        else:
            has_h = zi in (7, 8)
        if zi == 6:
            f = HYDROPHOBIC if all(z[j] == 6 for j in nbrs[i]) else 0
        elif zi in _HALOGENS:
            f = HYDROPHOBIC
        elif zi == 8:
            f = ACCEPTOR | (DONOR if has_h else 0)
        elif zi == 7:
            f = (DONOR if has_h else 0) | (ACCEPTOR if name in TABLES["nitrogen_acceptors"].get(res, ()) else 0)
        flags[i] = f
    return radii, flags


def type_receptor_graph(graph):
    """(radii, flags) of a complex graph's atom nodes; the bonds are perceived on the graph's own atom positions."""
    x = torch.as_tensor(graph["atom"].x).long().numpy()
    z = [ATOMIC_NUMS[i] if ATOMIC_NUMS[i] != "misc" else 0 for i in x[:, 1].tolist()]
    return receptor_types(x[:, 0], z, x[:, 3], torch.as_tensor(graph["atom"].pos).double().numpy())


def typed_receptor(pdb_text: str, original_center) -> TypedReceptor:
    """Every atom of a PDB's first model (hydrogens and hetero atoms included, untyped where the tables say so), shifted into a graph's
    frame (coordinates - original_center), with its types.  Residue and atom names go through the graph's vocabularies
    (inputs.rec_atom_features), so an atom gets the type it has as a graph node."""
    res_i, z, name_i, coords = [], [], [], []
    for r in parse_pdb(pdb_text):
        for a in r.atoms:
            element = "C" if a.element == "CD" else a.element
            res_i.append(safe_index(AMINO_ACIDS, r.resname))
            z.append(ATOMIC_NUMBER.get(element.upper(), 0))
            name_i.append(safe_index(ATOM_TYPE_3, a.name))
            coords.append(a.coord)
    c = np.asarray(original_center, dtype=np.float64).reshape(1, 3)
    coords = (np.asarray(coords, dtype=np.float64).reshape(-1, 3) - c).astype(np.float32)
    radii, flags = receptor_types(res_i, z, name_i, coords)
    return TypedReceptor(coords, radii, flags)


def typed_tables(graph, receptor, drop_untyped_graph_atoms: bool = False, expects: str = "a TypedReceptor"):
    """The host tables of a complex's typed atoms: ({"lig_r" [n] fp32, "lig_f" [n] uint8, "rec" [m', 3] fp32, "rec_r" [m'] fp32, "rec_f"
    [m'] uint8}, keep [m] bool, the typed ones of all m receptor atoms).  receptor: "graph" (the graph's atom nodes) or a TypedReceptor
    in the graph's frame; `expects` names the other form in the ValueError of anything else."""
    lig_r, lig_f = type_ligand(graph)
    if isinstance(receptor, str):
        if receptor != "graph":
            raise ValueError(f"receptor: 'graph' or {expects}, got {receptor!r}")
        rec_r, rec_f = type_receptor_graph(graph)
        rec = torch.as_tensor(graph["atom"].pos).float().reshape(-1, 3).numpy()
    else:
        if not isinstance(receptor, TypedReceptor):
            raise ValueError(f"receptor: 'graph' or {expects}, got {type(receptor).__name__}")
        rec = np.asarray(receptor.coords, dtype=np.float32).reshape(-1, 3)
        rec_r, rec_f = np.asarray(receptor.radii, dtype=np.float32), np.asarray(receptor.flags, dtype=np.uint8)
    keep = np.asarray(rec_r) >= 0
    # Untyped atoms take part in nothing and are dropped - except, for the scorer, those of a graph receptor: a per-sample atom_pos has
    # all n_a rows and is handed to the kernel as it is.  The profiler drops them there too and indexes atom_pos with `keep`.
    if drop_untyped_graph_atoms or not isinstance(receptor, str):
        rec, rec_r, rec_f = rec[keep], rec_r[keep], rec_f[keep]
    tables = {"lig_r": lig_r, "lig_f": lig_f, "rec": rec, "rec_r": rec_r, "rec_f": rec_f}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tables.items()}, keep


# ---------------------------------------------------------------------------------------------- the PyTorch fp64 form
def _ramp(s, good, bad):
    return torch.where(s <= good, torch.ones_like(s), torch.where(s < bad, (bad - s) / (bad - good), torch.zeros_like(s)))


def _pair_sums(diff, rsum, ok, hyd, hb, c: ScoreConfig, with_grad: bool):
    """diff [..., a, b, 3] fp64 (first atom - second), rsum / ok / hyd / hb [a, b] -> (the four sums over the last two pair axes
    [..., 4], d(weighted energy)/d(first atom) summed over the second [..., a, 3] or None)."""
    d2 = diff.pow(2).sum(-1)
    d = d2.sqrt()
    inside = ok & ~(d2 >= c.cutoff * c.cutoff)           # written so that a NaN distance goes through
    s = d - rsum
    u = (s - c.gauss_offset) / c.gauss_width
    ga = torch.exp(-(u * u))
    zero = torch.zeros_like(d)
    neg = inside & (s < 0)
    in_h, in_b = inside & hyd, inside & hb
    terms = torch.stack([torch.where(inside, ga, zero).sum((-1, -2)), torch.where(neg, s * s, zero).sum((-1, -2)),
                         torch.where(in_h, _ramp(s, c.hydrophobic_good, c.hydrophobic_bad), zero).sum((-1, -2)),
                         torch.where(in_b, _ramp(s, c.hbond_good, c.hbond_bad), zero).sum((-1, -2))], -1)
    if not with_grad:
        return terms, None
    de = torch.where(inside, c.w_gauss * (ga * (-2.0 * u / c.gauss_width)), zero)
    de = de + torch.where(neg, c.w_repulsion * (2.0 * s), zero)
    slope_h = torch.full_like(d, -c.w_hydrophobic / (c.hydrophobic_bad - c.hydrophobic_good))
    slope_b = torch.full_like(d, -c.w_hbond / (c.hbond_bad - c.hbond_good))
    de = de + torch.where(in_h & (s > c.hydrophobic_good) & (s < c.hydrophobic_bad), slope_h, zero)
    de = de + torch.where(in_b & (s > c.hbond_good) & (s < c.hbond_bad), slope_b, zero)
    unit = torch.where((d != 0).unsqueeze(-1), diff / d.unsqueeze(-1), torch.zeros_like(diff))
    return terms, (de.unsqueeze(-1) * unit).sum(-2)


def _weighted(t, c: ScoreConfig):
    return c.w_gauss * t[..., 0] + c.w_repulsion * t[..., 1] + c.w_hydrophobic * t[..., 2] + c.w_hbond * t[..., 3]


def score_torch(x, lig_r, lig_f, rec, rec_r, rec_f, self_pairs, config: ScoreConfig, tor_divisor: float = 1.0, with_grad: bool = False):
    """([S, 7] fp64 = gauss, repulsion, hydrophobic, hbond, inter, intra, total; [S, n, 3] fp64 gradient or None) of fp32 poses x - the
    definition of the module docstring on host tensors.  rec [m, 3] or [S, m, 3]."""
    c = config
    S, n = x.shape[0], x.shape[1]
    m = rec.shape[-2]
    x64, lr, rr = x.double(), lig_r.double(), rec_r.double()
    lf, rf = lig_f.to(torch.int64), rec_f.to(torch.int64)
    e = torch.zeros(S, 7, dtype=torch.float64)
    g = torch.zeros(S, n, 3, dtype=torch.float64) if with_grad else None

    def tables(ra, fa, rb, fb):
        ok = (ra[:, None] >= 0) & (rb[None, :] >= 0)
        hyd = (fa[:, None] & fb[None, :] & 1) != 0
        hb = ((((fa[:, None] >> 1) & (fb[None, :] >> 2)) | ((fa[:, None] >> 2) & (fb[None, :] >> 1))) & 1) != 0
        return ra[:, None] + rb[None, :], ok, hyd, hb

    cross = tables(lr, lf, rr, rf)
    sp = None
    if self_pairs is not None and n > 1:
        rs, ok, hyd, hb = tables(lr, lf, lr, lf)
        sp = (rs, ok & (self_pairs.bool() | self_pairs.bool().T), hyd, hb)
    chunk = max(1, (1 << 22) // max(1, n * max(m, n) * 3))
    for s0 in range(0, S, chunk):
        xs = x64[s0:s0 + chunk]
        if m > 0:
            r = (rec[None] if rec.dim() == 2 else rec[s0:s0 + chunk]).double()
            t, gc = _pair_sums(xs[:, :, None, :] - r[:, None, :, :], *cross, c, with_grad)
            e[s0:s0 + chunk, :4] = t
            if with_grad:
                g[s0:s0 + chunk] += gc
        if sp is not None:
            t, gs = _pair_sums(xs[:, :, None, :] - xs[:, None, :, :], *sp, c, with_grad)
            e[s0:s0 + chunk, 5] = _weighted(0.5 * t, c)          # every pair is met from both ends
            if with_grad:
                g[s0:s0 + chunk] += gs
    e[:, 4] = _weighted(e[:, :4], c)
    e[:, 6] = e[:, 4] / tor_divisor
    return e, g


# ---------------------------------------------------------------------------------------------- scorer
class PoseScorer:
    """The Vinardo-form score of the poses of one complex (see the module docstring).

    graph, device: as PoseEvaluator.  receptor: "graph" (the graph's atom nodes; each sample's own atom_pos when one is handed in:
    flexible runs) or a TypedReceptor in the graph's frame, e.g. typed_receptor(pdb_text, graph.original_center), the static full
    receptor of rigid runs (its untyped atoms are dropped here: they take part in nothing)."""

    def __init__(self, graph, device="cpu", receptor="graph", config: Optional[ScoreConfig] = None):
        self.config = (config or ScoreConfig()).check()
        self.device = torch.device(device)
        self.n = int(graph["ligand"].pos.shape[0])
        self.n_a = int(graph["atom"].pos.shape[0])
        self.receptor_from_graph = isinstance(receptor, str)
        cpu, _ = typed_tables(graph, receptor)
        bonds, mask_rotate = ligand_torsions(graph)
        self.n_tor = int(bonds.shape[0])
        self.tor_divisor = 1.0 + self.config.w_torsion * self.n_tor
        self.self_pairs = build_self_pairs(self.n, torch.as_tensor(graph["ligand", "ligand"].edge_index).numpy(), mask_rotate.numpy())
        cpu["pairs"] = self.self_pairs.contiguous()
        self._cpu = cpu
        self._dev = cpu if self.device.type == "cpu" else {k: v.to(self.device) for k, v in cpu.items()}

    def _check(self, lig_pos, atom_pos):
        check_poses(self.n, self.n_a, self.device, lig_pos, atom_pos, "scorer")

    def score(self, lig_pos: torch.Tensor, atom_pos: Optional[torch.Tensor] = None, with_grad: bool = False) -> PoseScores:
        """lig_pos [S, n, 3] (flexible runs: atom_pos [S, n_a, 3], each sample's own receptor; used by a graph receptor only) ->
        PoseScores on the poses' device."""
        self._check(lig_pos, atom_pos)
        x = lig_pos.float().contiguous()
        t = self._dev if x.is_cuda else self._cpu
        rec = atom_pos.float().contiguous() if (atom_pos is not None and self.receptor_from_graph) else t["rec"]
        if x.is_cuda:
            from . import launch as LA
            with torch.cuda.device(x.device):
                e, g = LA.pose_score(x, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], self.config, self.tor_divisor, t["pairs"],
                                     with_grad=with_grad)
        else:
            e, g = score_torch(x, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], t["pairs"], self.config, self.tor_divisor, with_grad)
        return PoseScores(e[:, :4].contiguous(), e[:, 4].contiguous(), e[:, 5].contiguous(), e[:, 6].contiguous(), g)


def rank_order(total: torch.Tensor) -> torch.Tensor:
    """Sample indices by ascending total; ties in sample order, NaN last (in sample order)."""
    key = torch.where(torch.isnan(total), torch.full_like(total, float("inf")), total)
    return torch.argsort(key, stable=True)
