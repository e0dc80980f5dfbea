"""Per-residue interaction profile and interaction fingerprints of poses: which residues a pose touches, and how.  The pair terms
of the Vinardo-form score (scoring.py) are summed per residue instead of over the whole receptor, and three bits per residue are
read off the sums.  This docstring is the definition; csrc/ddp_profile.hip and `profile_torch` below follow it.

Inputs.
    poses x [S, n, 3] fp32; ligand radii and flags [n] (scoring.type_ligand)
    a typed receptor rec [m, 3] or [S, m, 3] fp32 with radii and flags [m] (the types of scoring.py; a radius below 0: untyped)
    res_ptr [R + 1] int32, non-decreasing, res_ptr[0] = 0, res_ptr[R] = m: residue r owns the receptor atoms
        res_ptr[r] .. res_ptr[r+1] - 1; a residue may be empty
    the constants of a scoring.ScoreConfig, and ProfileConfig(contact_distance=4.5)

Pair terms, over ligand atom i and receptor atom j, both typed, with centre distance d < 8 A (strict); s = d - R_i - R_j:
    gauss       = exp(-(s / 0.8)^2)
    repulsion   = s^2 if s < 0, else 0
    hydrophobic = (both atoms hydrophobic)              1 for s <= 0, linear to 0 at s = 2.5
    hbond       = (a donor-acceptor pair, either way)   1 for s <= -0.6, linear to 0 at s = 0

Per sample s and residue r, over the pairs (ligand atom i, atom j of residue r) that are both typed and have d < cutoff (strict); all
arithmetic is fp64 on the fp32 inputs (converted first), as in scoring.py:
    terms[s, r, k], k = 0..3   the four unweighted sums gauss, repulsion, hydrophobic, hbond
    energy[s, r]               w_gauss terms0 + w_repulsion terms1 + w_hydrophobic terms2 + w_hbond terms3: the residue's share of
                               `inter`; summed over r it is `inter` of PoseScorer
    pairs[s, r]                the number of such pairs, an exact integer
    d_min[s, r]                the smallest d among them, +inf if there are none
    bits[s, r] (uint8)         bit 0 CONTACT iff d_min < contact_distance
                               bit 1 HYDROPHOBIC iff terms2 > 0
                               bit 2 HBOND iff terms3 > 0

Poison rule (local and cheap).  If any coordinate of a typed ligand atom of sample s is non-finite, every residue of that sample is
poisoned.  If only a typed atom of residue r (in that sample's receptor) has a non-finite coordinate, that residue of that sample is
poisoned.  A poisoned entry has terms, energy and d_min = NaN, pairs = 0 and bits = 0.  No other sample or residue is affected.

On the bits, as 0/1 vectors over 3R positions:
    tanimoto(a, b)   = |a & b| / |a | b|, and 1.0 where both are empty
    recovery(a, ref) = |a & ref| / |ref|, and NaN where ref is empty
    frequency [R, 3] = the share of the samples that have each bit set

What it is not.  It inherits every limit of the score: no directional hydrogen bonds, no hydrogens, no metals, not validated against
smina, Vina, PLIP or ProLIF.  There are no pi-stacking, salt-bridge or water terms.  The HYDROPHOBIC bit is broad: any hydrophobic pair
within 2.5 A of surface contact sets it.  contact_distance is the customary 4.5 A; it is untuned.

Device tensors go through csrc/ddp_profile.hip (ddp_pose_profile: one workgroup per sample, one launch); CPU tensors through the
PyTorch fp64 form below (`profile_torch`), chunked over the samples.  The bit arithmetic is plain torch on the poses' device."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .inputs import AMINO_ACIDS, parse_pdb
from .pose_args import check_poses
from .scoring import ScoreConfig, TypedReceptor, _ramp, _weighted, typed_tables

CONTACT, HYDROPHOBIC_BIT, HBOND_BIT = 1, 2, 4


@dataclass
class ProfileConfig:
    """contact_distance: the CONTACT bit is set iff the closest pair of the residue is nearer than this (angstrom, centre to centre)."""
    contact_distance: float = 4.5

    def check(self):
        if not (self.contact_distance > 0 and np.isfinite(self.contact_distance)):
            raise ValueError("ProfileConfig: contact_distance must be positive and finite")
        return self


# ---------------------------------------------------------------------------------------------- residue tables
@dataclass
class ResidueTable:
    """The residues of a receptor's atoms: residue r owns the atoms ptr[r] .. ptr[r + 1] - 1 and is called labels[r]."""
    ptr: np.ndarray          # [R + 1] int32, non-decreasing, ptr[0] = 0, ptr[R] = the number of atoms
    labels: List[str]        # [R]

    def check(self, m: Optional[int] = None):
        p = np.asarray(self.ptr)
        if p.ndim != 1 or len(p) != len(self.labels) + 1 or p[0] != 0 or bool((np.diff(p) < 0).any()) or (m is not None and p[-1] != m):
            raise ValueError("ResidueTable: ptr must be [R + 1], non-decreasing, start at 0 and end at the number of atoms")
        return self

    def index(self) -> np.ndarray:
        """The residue of every atom, [m] int64."""
        return np.repeat(np.arange(len(self.labels), dtype=np.int64), np.diff(np.asarray(self.ptr, dtype=np.int64)))

    @staticmethod
    def from_index(index, labels: Sequence[str]) -> "ResidueTable":
        """From the residue of every atom; the atoms of a residue have to be contiguous and the residues in order."""
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        R = len(labels)
        if len(index) and (bool((np.diff(index) < 0).any()) or index[0] < 0 or index[-1] >= R):
            raise ValueError("the residue index of the receptor atoms must be non-decreasing and lie in [0, R)")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(index, minlength=R))]).astype(np.int32)
        return ResidueTable(ptr, list(labels))

    def keep(self, mask) -> "ResidueTable":
        """The table of the atoms mask [m] keeps; a residue may become empty."""
        mask = np.asarray(mask, dtype=bool)
        return ResidueTable.from_index(self.index()[mask], self.labels)


def receptor_residues(pdb_text: str) -> ResidueTable:
    """The residue of every atom of scoring.typed_receptor(pdb_text, ...), in its atom order (the same parse_pdb walk: hydrogens and
    hetero residues included).  Labels: "{chain}:{resname}{resseq}{icode}"."""
    sizes, labels = [], []
    for r in parse_pdb(pdb_text):
        sizes.append(len(r.atoms))
        labels.append(f"{r.chain}:{r.resname}{r.resseq}{r.icode.strip()}")
    return ResidueTable(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), labels)


def graph_residues(graph) -> ResidueTable:
    """The residue node of every atom node of a complex graph (("atom", "receptor").edge_index[1]).  Labels: "{residue node}:{resname}",
    the residue name from atom.x[:, 0] (a residue node without atoms: from receptor.x[:, 0])."""
    index = torch.as_tensor(graph["atom", "receptor"].edge_index)[1].long().numpy()
    R = int(graph["receptor"].x.shape[0])
    name_of = torch.as_tensor(graph["receptor"].x)[:, 0].long().tolist()
    ax = torch.as_tensor(graph["atom"].x)[:, 0].long().tolist()
    for a in range(len(index) - 1, -1, -1):
        if 0 <= index[a] < R:
            name_of[int(index[a])] = ax[a]
    return ResidueTable.from_index(index, [f"{r}:{AMINO_ACIDS[int(name_of[r])]}" for r in range(R)])


# ---------------------------------------------------------------------------------------------- the bits
def _bit_vectors(bits: torch.Tensor) -> torch.Tensor:
    """bits [..., R] uint8 -> 0/1 vectors [..., 3R] fp32."""
    b = bits.to(torch.int64)
    return torch.stack([(b >> k) & 1 for k in range(3)], -1).reshape(*bits.shape[:-1], -1).float()


def tanimoto(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [S, R], b [T, R] uint8 -> [S, T] fp64: |a & b| / |a | b| over the 3R bit positions, 1.0 where both are empty.  The counts go
    through an fp32 matmul, exact below 2^24."""
    va, vb = _bit_vectors(a), _bit_vectors(b)
    both = (va @ vb.T).double()
    either = va.sum(-1).double()[:, None] + vb.sum(-1).double()[None, :] - both
    return torch.where(either == 0, torch.ones_like(both), both / torch.where(either == 0, torch.ones_like(either), either))


def recovery(a: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """a [S, R], ref [R] uint8 -> [S] fp64: |a & ref| / |ref|, NaN where ref is empty."""
    va, vr = _bit_vectors(a), _bit_vectors(ref.reshape(1, -1))
    return (va @ vr.T).double()[:, 0] / vr.sum().double()


@dataclass
class InteractionProfile:
    """What InteractionProfiler.profile returns, in the order of the poses handed in, on their device (see the module docstring)."""
    terms: torch.Tensor       # [S, R, 4] fp64: gauss, repulsion, hydrophobic, hbond
    energy: torch.Tensor      # [S, R] fp64
    d_min: torch.Tensor       # [S, R] fp64
    pairs: torch.Tensor       # [S, R] int64
    bits: torch.Tensor        # [S, R] uint8: CONTACT | HYDROPHOBIC_BIT | HBOND_BIT
    labels: List[str]         # [R]

    def _map(self, fn) -> "InteractionProfile":
        return InteractionProfile(fn(self.terms), fn(self.energy), fn(self.d_min), fn(self.pairs), fn(self.bits), self.labels)

    def cpu(self) -> "InteractionProfile":
        return self._map(lambda t: t.cpu())

    def index(self, order) -> "InteractionProfile":
        return self._map(lambda t: t[order.to(t.device)])

    def similarity(self) -> torch.Tensor:
        """[S, S] fp64: the Tanimoto similarity of every pair of poses."""
        return tanimoto(self.bits, self.bits)

    def tanimoto_to(self, other_bits: torch.Tensor) -> torch.Tensor:
        """[S] fp64: the Tanimoto similarity of every pose to other_bits [R]."""
        return tanimoto(self.bits, other_bits.to(self.bits.device).reshape(1, -1))[:, 0]

    def recovery(self, ref_bits: torch.Tensor) -> torch.Tensor:
        """[S] fp64: the share of the set bits of ref_bits [R] that every pose has too; NaN where ref_bits is empty."""
        return recovery(self.bits, ref_bits.to(self.bits.device))

    def frequency(self) -> torch.Tensor:
        """[R, 3] fp64: the share of the poses with CONTACT, HYDROPHOBIC, HBOND set."""
        S, R = self.bits.shape
        v = _bit_vectors(self.bits).reshape(S, R, 3).double()
        return v.sum(0) / S if S else torch.full((R, 3), float("nan"), dtype=torch.float64, device=self.bits.device)


# ---------------------------------------------------------------------------------------------- the PyTorch fp64 form
def profile_torch(x, lig_r, lig_f, rec, rec_r, rec_f, res_ptr, config: ScoreConfig, contact_distance: float = 4.5):
    """(profile [S, R, 7] fp64 = gauss, repulsion, hydrophobic, hbond, energy, d_min, pairs; bits [S, R] uint8) of fp32 poses x - the
    definition of the module docstring on host tensors.  rec [m, 3] or [S, m, 3]; res_ptr [R + 1]."""
    c = config
    S, n = x.shape[0], x.shape[1]
    m = rec.shape[-2]
    ptr = torch.as_tensor(res_ptr).to(torch.int64).reshape(-1)
    R = ptr.shape[0] - 1
    res = torch.repeat_interleave(torch.arange(R, dtype=torch.int64), ptr[1:] - ptr[:-1])        # [m]
    lr, rr = lig_r.double(), rec_r.double()
    lf, rf = lig_f.to(torch.int64), rec_f.to(torch.int64)
    ok = (lr[:, None] >= 0) & (rr[None, :] >= 0)
    hyd = (lf[:, None] & rf[None, :] & 1) != 0
    hb = ((((lf[:, None] >> 1) & (rf[None, :] >> 2)) | ((lf[:, None] >> 2) & (rf[None, :] >> 1))) & 1) != 0
    rsum = lr[:, None] + rr[None, :]
    prof = torch.zeros(S, R, 7, dtype=torch.float64)
    prof[:, :, 5] = float("inf")
    bits = torch.zeros(S, R, dtype=torch.uint8)
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    chunk = max(1, (1 << 22) // max(1, n * max(m, 1) * 3))
    for s0 in range(0, S, chunk):
        xs = x[s0:s0 + chunk].double()
        B = xs.shape[0]
        r = (rec[None].expand(B, -1, -1) if rec.dim() == 2 else rec[s0:s0 + chunk]).double()
        # poison: a non-finite coordinate of a typed atom; such an atom is moved to the origin for the arithmetic and its entries are
        # overwritten at the end, so that no other entry sees it
        lig_atom_bad = ~torch.isfinite(xs).all(-1) & (lr >= 0)[None]                           # [B, n]
        rec_atom_bad = ~torch.isfinite(r).all(-1) & (rr >= 0)[None]                            # [B, m]
        xs = torch.where(lig_atom_bad[..., None], torch.zeros_like(xs), xs)
        r = torch.where(rec_atom_bad[..., None], torch.zeros_like(r), r)
        poisoned = lig_atom_bad.any(1)[:, None].expand(B, R).clone()
        if m > 0:
            poisoned |= torch.zeros(B, R, dtype=torch.float64).index_add_(1, res, rec_atom_bad.double()) > 0
            d2 = (xs[:, :, None, :] - r[:, None, :, :]).pow(2).sum(-1)                         # [B, n, m]
            d = d2.sqrt()
            inside = ok[None] & (d2 < c.cutoff * c.cutoff)
            sd = d - rsum
            u = (sd - c.gauss_offset) / c.gauss_width
            zero = torch.zeros_like(d)
            per_atom = torch.stack([torch.where(inside, torch.exp(-(u * u)), zero).sum(1),
                                    torch.where(inside & (sd < 0), sd * sd, zero).sum(1),
                                    torch.where(inside & hyd[None], _ramp(sd, c.hydrophobic_good, c.hydrophobic_bad), zero).sum(1),
                                    torch.where(inside & hb[None], _ramp(sd, c.hbond_good, c.hbond_bad), zero).sum(1),
                                    inside.double().sum(1)], -1)                                # [B, m, 5]: sums over the ligand atoms
            t = torch.zeros(B, R, 5, dtype=torch.float64).index_add_(1, res, per_atom)
            near = torch.where(inside, d, inf).amin(1)                                         # [B, m]
            dmin = torch.full((B, R), float("inf"), dtype=torch.float64).scatter_reduce_(1, res[None].expand(B, -1), near, "amin")
            prof[s0:s0 + B, :, :4] = t[..., :4]
            prof[s0:s0 + B, :, 4] = _weighted(t[..., :4], c)
            prof[s0:s0 + B, :, 5] = dmin
            prof[s0:s0 + B, :, 6] = t[..., 4]
        p = prof[s0:s0 + B]
        b = ((p[..., 5] < contact_distance).to(torch.uint8) * CONTACT + (p[..., 2] > 0).to(torch.uint8) * HYDROPHOBIC_BIT
             + (p[..., 3] > 0).to(torch.uint8) * HBOND_BIT)
        p[..., :6] = torch.where(poisoned[..., None], torch.full_like(p[..., :6], float("nan")), p[..., :6])
        p[..., 6] = torch.where(poisoned, torch.zeros_like(p[..., 6]), p[..., 6])
        bits[s0:s0 + B] = torch.where(poisoned, torch.zeros_like(b), b)
    return prof, bits


# ---------------------------------------------------------------------------------------------- profiler
class InteractionProfiler:
    """The per-residue interaction profile of the poses of one complex (see the module docstring).

    graph, device: as PoseScorer.  receptor: "graph" (the graph's atom nodes with the residues of graph_residues; each sample's own
    atom_pos when one is handed in: flexible runs) or a pair (TypedReceptor, ResidueTable) in the graph's frame, e.g.
    (typed_receptor(pdb_text, graph.original_center), receptor_residues(pdb_text)): the static full receptor of rigid runs.  Untyped
    receptor atoms are dropped here (they take part in nothing) and the residue table is rebuilt: a residue may become empty, it
    keeps its row.  ValueError if the residue index of the atoms is not non-decreasing."""

    def __init__(self, graph, device="cpu", receptor="graph", config: Optional[ProfileConfig] = None,
                 score_config: Optional[ScoreConfig] = None):
        self.config = (config or ProfileConfig()).check()
        self.score_config = (score_config or ScoreConfig()).check()
        self.device = torch.device(device)
        self.n = int(graph["ligand"].pos.shape[0])
        self.n_a = int(graph["atom"].pos.shape[0])
        self.receptor_from_graph = isinstance(receptor, str)
        pair = "(TypedReceptor, ResidueTable)"
        if not self.receptor_from_graph and not (isinstance(receptor, (tuple, list)) and len(receptor) == 2
                                                 and isinstance(receptor[0], TypedReceptor) and isinstance(receptor[1], ResidueTable)):
            raise ValueError(f"receptor: 'graph' or {pair}, got {type(receptor).__name__}")
        # untyped atoms are dropped; the rows a per-sample atom_pos keeps are `self.keep`
        cpu, keep = typed_tables(graph, receptor if self.receptor_from_graph else receptor[0], drop_untyped_graph_atoms=True, expects=pair)
        table = graph_residues(graph) if self.receptor_from_graph else receptor[1]
        table.check(len(keep))
        self.keep = torch.from_numpy(np.nonzero(keep)[0])
        self.table = table.keep(keep)
        self.labels = list(self.table.labels)
        self.n_res = len(self.labels)
        cpu.update(ptr=torch.from_numpy(np.ascontiguousarray(self.table.ptr, dtype=np.int32)), keep=self.keep)
        self._cpu = cpu
        self._dev = cpu if self.device.type == "cpu" else {k: v.to(self.device) for k, v in cpu.items()}

    def _check(self, lig_pos, atom_pos):
        check_poses(self.n, self.n_a, self.device, lig_pos, atom_pos, "profiler")

    def profile(self, lig_pos: torch.Tensor, atom_pos: Optional[torch.Tensor] = None) -> InteractionProfile:
        """lig_pos [S, n, 3] (flexible runs: atom_pos [S, n_a, 3], each sample's own receptor; used by a graph receptor only) ->
        InteractionProfile on the poses' device."""
        self._check(lig_pos, atom_pos)
        x = lig_pos.float().contiguous()
        t = self._dev if x.is_cuda else self._cpu
        rec = t["rec"]
        if atom_pos is not None and self.receptor_from_graph:
            rec = atom_pos.float()[:, t["keep"]].contiguous()
        if x.is_cuda:
            from . import launch as LA
            with torch.cuda.device(x.device):
                p, b = LA.pose_profile(x, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], t["ptr"], self.score_config,
                                       self.config.contact_distance)
        else:
            p, b = profile_torch(x, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], t["ptr"], self.score_config,
                                 self.config.contact_distance)
        return InteractionProfile(p[..., :4].contiguous(), p[..., 4].contiguous(), p[..., 5].contiguous(),
                                  p[..., 6].to(torch.int64), b, self.labels)
