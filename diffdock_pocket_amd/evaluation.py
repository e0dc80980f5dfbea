"""Evaluation of sampled poses against a reference pose: the per-complex scoring of reference evaluate_files.py:151-340.

  rmsd        symmetry-corrected ligand RMSD (utils/utils.py:116-130, spyrmsd `symmrmsd` with its defaults: no centring, no
              alignment, the minimum over the automorphisms of the heavy-atom graph by element + adjacency; bond orders unused)
  rmsd_plain  the RMSD without symmetry (the reference's fallback, evaluate_files.py:150-154)
  centroid    distance of the ligand centroid to the reference centroid
  min_cross   minimum ligand-receptor distance;  min_self: minimum ligand-ligand distance over i != j
  clashes     receptor-ligand steric clashes (datasets/steric_clash.py:99-136: d < r_vdw1 + r_vdw2 - 2 * 0.4, receptor H excluded)
  sc_rmsd     RMSD of the flexible residues' side-chain heavy atoms (evaluate_files.py:200-237; flexible runs only)

`PoseEvaluator` is built once per complex from the input graph (its ligand pose - and atom positions - are the reference pose, as
the crystal ligand is for PDBBind) and scores the [S, n, 3] poses of a Sampler.  Device tensors go through the HIP kernels of
csrc/ddp_eval.hip (two launches, one workgroup per sample); CPU tensors through `_rmsd_torch` / `_contacts_torch`, the same
arithmetic in PyTorch (the CPU tests and the csv driver with a stub model).  `summarize` turns the ranked metrics of many complexes
into the reference's percentages.

Without a known pose: `PoseEvaluator.pairwise_rmsd` is the same symmetry-corrected RMSD between every pair of samples
(ddp_pose_pairwise_rmsd / `_pairwise_torch`) and `PoseEvaluator.cluster` groups the samples into binding modes by greedy leader
clustering in ranked order (ddp_pose_cluster / `_cluster_torch`) -> `PoseClusters`."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .inputs import ATOM_TYPE_3, _SYMBOLS
from .pose_args import check_poses

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
OVERLAP_DISTANCE = 0.4
_BACKBONE = {ATOM_TYPE_3.index(a) for a in ("CA", "N", "C", "O", "OXT")}


# ---------------------------------------------------------------------------------------------- van der Waals radii
def _load_radii():
    with open(os.path.join(ASSETS, "vdw_radii.json")) as f:
        d = json.load(f)
    return {k.upper(): float(v) for k, v in d["radii"].items()}, float(d["default"])


VDW_RADII, VDW_DEFAULT = _load_radii()


def element_symbol(atomic_num: int) -> Optional[str]:
    return _SYMBOLS[atomic_num - 1] if 1 <= atomic_num <= len(_SYMBOLS) else None


def vdw_radius(element: Union[str, int, None]) -> float:
    """Radius of an element symbol or atomic number; 2.0 A for every element the table does not list (metals, unknown)."""
    if isinstance(element, (int, np.integer)):
        element = element_symbol(int(element))
    return VDW_RADII.get(str(element).strip().upper(), VDW_DEFAULT) if element is not None else VDW_DEFAULT


def _is_h(element) -> bool:
    return element == 1 if isinstance(element, (int, np.integer)) else str(element).strip().upper() == "H"


# ---------------------------------------------------------------------------------------------- graph automorphisms
def ligand_automorphisms(atomic_num, edge_index, max_count: int = 100_000) -> Tuple[np.ndarray, bool]:
    """Every permutation of the ligand graph that preserves element and adjacency, as int32 [P, n]: row p maps atom i of a pose to
    atom perm[p, i] of the reference.  Rows are sorted lexicographically (the identity first).  Colour refinement by element and
    neighbour colours, then backtracking over the refined classes in breadth-first atom order.  More than `max_count`: returns
    (identity only, False) - the reference's fallback to the plain RMSD when the symmetry search fails (evaluate_files.py:150-154);
    otherwise (perms, True)."""
    z = np.asarray(atomic_num, dtype=np.int64).reshape(-1)
    n = len(z)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    adj = [set() for _ in range(n)]
    for a, b in ei.T:
        if a != b:
            adj[int(a)].add(int(b))
            adj[int(b)].add(int(a))
    ident = np.arange(n, dtype=np.int32)[None]
    if n == 0:
        return ident, True
    # colour refinement: (colour, sorted neighbour colours) until the number of classes is stable
    col = np.unique(z, return_inverse=True)[1].tolist()
    while True:
        sig = [(col[i], tuple(sorted(col[j] for j in adj[i]))) for i in range(n)]
        keys = {s: k for k, s in enumerate(sorted(set(sig)))}
        new = [keys[s] for s in sig]
        if len(keys) == len(set(col)):
            col = new
            break
        col = new
    classes: Dict[int, List[int]] = {}
    for i in range(n):
        classes.setdefault(col[i], []).append(i)
    # breadth-first order, each component started at its atom of the smallest class (lowest index on ties)
    key = lambda i: (len(classes[col[i]]), i)     # noqa: E731
    order, seen = [], [False] * n
    for start in sorted(range(n), key=key):
        if seen[start]:
            continue
        seen[start] = True
        q = [start]
        while q:
            a = q.pop(0)
            order.append(a)
            for b in sorted(adj[a], key=key):
                if not seen[b]:
                    seen[b] = True
                    q.append(b)
    pos = {a: k for k, a in enumerate(order)}
    earlier = [[c for c in adj[a] if pos[c] < k] for k, a in enumerate(order)]
    perm, used, out = [-1] * n, [False] * n, []
    # iterative backtracking: stack[k] = index of the next candidate tried for order[k]
    stack, k = [0], 0
    while k >= 0:
        a = order[k]
        cands = classes[col[a]]
        ci = stack[k]
        if perm[a] >= 0:                  # undo the previous choice at this level
            used[perm[a]] = False
            perm[a] = -1
        found = False
        while ci < len(cands):
            b = cands[ci]
            ci += 1
            if used[b]:
                continue
            if all(perm[c] in adj[b] for c in earlier[k]) and sum(used[d] for d in adj[b]) == len(earlier[k]):
                found = True
                break
        stack[k] = ci
        if not found:
            stack.pop()
            k -= 1
            continue
        perm[a], used[b] = b, True
        if k == n - 1:
            out.append(list(perm))
            if len(out) > max_count:
                return ident, False
            continue                      # try the next candidate at the same level
        k += 1
        stack.append(0)
    arr = np.asarray(out, dtype=np.int32).reshape(-1, n)
    arr = arr[np.lexsort(arr.T[::-1])]
    return arr, True


# ---------------------------------------------------------------------------------------------- the PyTorch form
def _rmsd_torch(pred, ref, perms_pn, sel=None):
    """min_p sqrt(sum_i |pred[s, sel_i] - ref[perms[p, i]]|^2 / n) (fp32 differences, fp64 sums) and its p (ties: the lowest)."""
    x = pred if sel is None else pred[:, sel]
    S, n = x.shape[0], x.shape[1]
    best_v = torch.full((S,), float("inf"), dtype=torch.float64)
    best_p = torch.full((S,), -1, dtype=torch.int64)
    P = perms_pn.shape[0]
    chunk = max(1, (1 << 24) // max(1, S * n * 3))
    for p0 in range(0, P, chunk):
        rp = ref[perms_pn[p0:p0 + chunk].long()]                      # [c, n, 3]
        d = (x[:, None] - rp[None]).double()
        acc = (d * d).sum(-1).sum(-1)                                  # [S, c]
        v, i = acc.min(1)                                              # first minimum
        take = v < best_v
        best_v, best_p = torch.where(take, v, best_v), torch.where(take, i + p0, best_p)
    return torch.sqrt(best_v / n).float(), best_p.to(torch.int32)


def _pairwise_torch(pos, perms_pn, sel=None):
    """[S, S]: for i < j, _rmsd_torch of pose j against ref = the selected rows of pose i (the arithmetic and chunking of
    _rmsd_torch, one call per i); the lower triangle is a copy of the upper one, the diagonal is 0."""
    x = pos if sel is None else pos[:, sel]
    S = x.shape[0]
    dist = torch.zeros(S, S, dtype=torch.float32)
    for i in range(S - 1):
        dist[i, i + 1:] = _rmsd_torch(x[i + 1:], x[i], perms_pn)[0]
    return torch.triu(dist, 1) + torch.triu(dist, 1).T


def _cluster_torch(dist, order=None, cutoff=2.0):
    """Greedy leader clustering, the rule of ddp_pose_cluster on the host: (labels [S], reps [S], sizes [S], count), int32, reps and
    sizes -1 past `count`.  Walking `order` (None: 0 .. S-1), a pose without a label opens the next cluster and takes every pose that
    has no label yet and dist[rep, t] < cutoff (strict; NaN never joins), itself included."""
    S = dist.shape[0]
    d = dist.float()
    cut = torch.tensor(float(cutoff), dtype=torch.float32)
    labels, reps, sizes = (torch.full((S,), -1, dtype=torch.int32) for _ in range(3))
    count = 0
    for o in (range(S) if order is None else [int(v) for v in order]):
        if o < 0 or o >= S or labels[o] >= 0:
            continue
        join = (labels < 0) & (d[o] < cut)
        join[o] = True
        labels[join] = count
        reps[count], sizes[count] = o, int(join.sum())
        count += 1
    return labels, reps, sizes, count


def _contacts_torch(lig, lig_r, rec, rec_r, ref_c, overlap=OVERLAP_DISTANCE):
    """[S, 4] = clashes, min_cross, min_self, centroid (the arithmetic of ddp_pose_contacts: fp32 squared distances)."""
    S, n = lig.shape[0], lig.shape[1]
    m = rec.shape[-2]
    out = torch.empty(S, 4, dtype=torch.float32)
    t = lig_r[:, None] + rec_r[None, :] - 2.0 * overlap
    ok = (rec_r[None, :] >= 0) & (t > 0)
    chunk = max(1, (1 << 24) // max(1, n * max(m, 1) * 3))
    eye = torch.eye(n, dtype=torch.bool)
    for s0 in range(0, S, chunk):
        x = lig[s0:s0 + chunk]
        if m > 0:
            r = rec[None] if rec.dim() == 2 else rec[s0:s0 + chunk]
            d = x[:, :, None, :] - r[:, None, :, :]
            d2 = (d * d).sum(-1)                                        # [c, n, m]
            out[s0:s0 + chunk, 0] = (ok & (d2 < t * t)).sum((1, 2)).float()
            out[s0:s0 + chunk, 1] = d2.amin((1, 2)).sqrt()
        else:
            out[s0:s0 + chunk, 0], out[s0:s0 + chunk, 1] = 0.0, float("inf")
        ds = x[:, :, None, :] - x[:, None, :, :]
        s2 = (ds * ds).sum(-1).masked_fill(eye, float("inf"))
        out[s0:s0 + chunk, 2] = s2.amin((1, 2)).sqrt()
    out[:, 3] = (lig.double().mean(1) - ref_c.double()).norm(dim=1).float()
    return out


# ---------------------------------------------------------------------------------------------- evaluator
@dataclass
class PoseMetrics:
    """Per-sample metrics ([S] tensors, in the order of the poses handed to `evaluate`)."""
    rmsd: torch.Tensor
    rmsd_plain: torch.Tensor
    best_perm: torch.Tensor        # row of the automorphism table that gave `rmsd`
    centroid: torch.Tensor
    min_cross: torch.Tensor
    min_self: torch.Tensor
    clashes: torch.Tensor          # int32
    sc_rmsd: Optional[torch.Tensor] = None
    symmetry_corrected: bool = True

    def _map(self, fn):
        return PoseMetrics(**{f.name: (fn(getattr(self, f.name)) if isinstance(getattr(self, f.name), torch.Tensor)
                                       else getattr(self, f.name)) for f in fields(self)})

    def cpu(self) -> "PoseMetrics":
        return self._map(lambda t: t.cpu())

    def index(self, order) -> "PoseMetrics":
        return self._map(lambda t: t[order.to(t.device)])


@dataclass
class PoseClusters:
    """Binding modes of S poses (PoseEvaluator.cluster), in the order of the poses handed in.  Mode c is led by its representative,
    the best-ranked pose that no earlier mode took, and holds every later-ranked free pose closer to it than the cutoff: modes are
    numbered by the rank of their representative, mode 0 holds the top-ranked pose."""
    dist: torch.Tensor                     # [S, S] symmetry-corrected RMSD of every pair (symmetric bit for bit, zero diagonal)
    labels: torch.Tensor                   # [S] int32 mode of each pose
    representatives: torch.Tensor          # [S] int32 pose index leading each mode, -1 past the last mode
    sizes: torch.Tensor                    # [S] int32 members of each mode, -1 past the last mode
    rmsd_to_representative: torch.Tensor   # [S] dist[representative of the pose's mode, pose]
    symmetry_corrected: bool = True

    def cpu(self) -> "PoseClusters":
        return PoseClusters(**{f.name: (getattr(self, f.name).cpu() if isinstance(getattr(self, f.name), torch.Tensor)
                                        else getattr(self, f.name)) for f in fields(self)})

    @property
    def n_modes(self) -> int:
        return int((self.sizes >= 0).sum())

    def by_size(self) -> List[int]:
        """Mode indices, the largest first (ties: the lower index, i.e. the better-ranked representative)."""
        sizes = self.sizes.cpu().tolist()[: self.n_modes]
        return sorted(range(len(sizes)), key=lambda c: (-sizes[c], c))


class PoseEvaluator:
    """Scores poses of one complex against the pose of its input graph.

    graph: the HeteroBatch the Sampler was built from (ligand heavy atoms, pocket-centred).  Elements are read from the graph like
    datasets/steric_clash.py:79-96 does: ligand x[:, 0] + 1 and atom-node x[:, 1] + 1 are atomic numbers.
    receptor: "graph" - clashes against the graph's atom nodes (each sample's own atom_pos when evaluate() gets one: flexible runs);
    or (coords [m, 3], elements [m]) in the graph's frame - e.g. `full_receptor(pdb_text, graph.original_center)`, the reference's
    static full-receptor form for rigid runs.  Hydrogens of the receptor count for min_cross, never for clashes.
    Side-chain RMSD (flexible graphs): the non-backbone heavy atoms of every residue with a rotatable side-chain bond."""

    def __init__(self, graph, device="cpu", receptor="graph", max_automorphisms: int = 100_000, overlap: float = OVERLAP_DISTANCE):
        self.device = torch.device(device)
        self.overlap = float(overlap)
        lig = graph["ligand"]
        self.n = int(lig.pos.shape[0])
        z_lig = (torch.as_tensor(lig.x)[:, 0].long() + 1).tolist()
        perms, self.symmetry_corrected = ligand_automorphisms(z_lig, torch.as_tensor(graph["ligand", "ligand"].edge_index).numpy(),
                                                              max_automorphisms)
        self.n_perms = perms.shape[0]
        atom = graph["atom"]
        self.n_a = int(atom.pos.shape[0])
        ref_atom = torch.as_tensor(atom.pos).float().reshape(-1, 3)
        self.receptor_from_graph = isinstance(receptor, str)
        if self.receptor_from_graph:
            if receptor != "graph":
                raise ValueError(f"receptor: 'graph' or (coords, elements), got {receptor!r}")
            z_rec = (torch.as_tensor(atom.x)[:, 1].long() + 1).tolist()
            rec, rec_el = ref_atom, z_rec
        else:
            coords, rec_el = receptor
            rec = torch.as_tensor(np.asarray(coords, dtype=np.float32)).reshape(-1, 3)
            rec_el = list(rec_el)
            if len(rec_el) != rec.shape[0]:
                raise ValueError("receptor: one element per coordinate row")
        rec_r = torch.tensor([-1.0 if _is_h(e) else vdw_radius(e) for e in rec_el], dtype=torch.float32)
        ref_lig = torch.as_tensor(lig.pos).float().reshape(-1, 3)
        sc = self._sidechain_rows(graph)
        cpu = {"ref_lig": ref_lig.contiguous(), "ref_centroid": ref_lig.double().mean(0).float(),
               "perms": torch.from_numpy(perms), "perms_t": torch.from_numpy(np.ascontiguousarray(perms.T)),
               "ident": torch.arange(self.n, dtype=torch.int32)[:, None].contiguous(),
               "lig_r": torch.tensor([vdw_radius(int(z)) for z in z_lig], dtype=torch.float32),
               "rec": rec.contiguous(), "rec_r": rec_r, "sc_rows": sc}
        if sc is not None:
            cpu["sc_ref"] = ref_atom[sc.long()].contiguous()
            cpu["sc_ident"] = torch.arange(len(sc), dtype=torch.int32)[:, None].contiguous()
        self._cpu = cpu
        self._dev = cpu if self.device.type == "cpu" else {k: (v.to(self.device) if v is not None else None) for k, v in cpu.items()}

    @staticmethod
    def _sidechain_rows(graph) -> Optional[torch.Tensor]:
        if len(graph["flexResidues"]) == 0:
            return None
        fr = graph["flexResidues"]
        atom_res = torch.as_tensor(graph["atom", "receptor"].edge_index)[1].long()
        flex_res = set(atom_res[torch.as_tensor(fr.subcomponents).long()].tolist())
        x = torch.as_tensor(graph["atom"].x)
        rows = [a for a in range(x.shape[0]) if int(atom_res[a]) in flex_res and int(x[a, 3]) not in _BACKBONE and int(x[a, 1]) != 0]
        return torch.tensor(rows, dtype=torch.int32) if rows else None

    @staticmethod
    def full_receptor(pdb_text: str, original_center) -> Tuple[np.ndarray, List[str]]:
        """(coords, elements) of every atom of a PDB's first model, shifted into a graph's frame (coordinates - original_center)."""
        from .inputs import parse_pdb
        atoms = [a for r in parse_pdb(pdb_text) for a in r.atoms]
        c = np.asarray(original_center, dtype=np.float64).reshape(1, 3)
        return (np.array([a.coord for a in atoms], dtype=np.float64) - c).astype(np.float32), [a.element for a in atoms]

    def evaluate(self, lig_pos: torch.Tensor, atom_pos: Optional[torch.Tensor] = None) -> PoseMetrics:
        """lig_pos [S, n, 3] (and, for flexible runs, atom_pos [S, n_a, 3]) -> PoseMetrics of [S] tensors on the poses' device."""
        check_poses(self.n, self.n_a, None, lig_pos, atom_pos, "evaluator")      # the shapes; device poses: _evaluate_hip tests the device
        if lig_pos.is_cuda:
            return self._evaluate_hip(lig_pos, atom_pos)
        return self._evaluate_torch(lig_pos.float(), None if atom_pos is None else atom_pos.float())

    def _receptor(self, t, atom_pos):
        return atom_pos if (atom_pos is not None and self.receptor_from_graph) else t["rec"]

    def _evaluate_torch(self, lig, apos) -> PoseMetrics:
        t = self._cpu
        rmsd, best = _rmsd_torch(lig, t["ref_lig"], t["perms"])
        plain, _ = _rmsd_torch(lig, t["ref_lig"], t["ident"].T)
        c = _contacts_torch(lig, t["lig_r"], self._receptor(t, apos), t["rec_r"], t["ref_centroid"], self.overlap)
        sc = None
        if apos is not None and t["sc_rows"] is not None:
            sc, _ = _rmsd_torch(apos, t["sc_ref"], t["sc_ident"].T, sel=t["sc_rows"].long())
        return PoseMetrics(rmsd, plain, best, c[:, 3].contiguous(), c[:, 1].contiguous(), c[:, 2].contiguous(), c[:, 0].to(torch.int32), sc,
                           self.symmetry_corrected)

    def _evaluate_hip(self, lig, apos) -> PoseMetrics:
        from . import launch as LA
        self._check_lig(lig)
        t = self._dev
        with torch.cuda.device(lig.device):
            lig = lig.float().contiguous()
            apos = None if apos is None else apos.float().contiguous()
            rmsd, best = LA.pose_rmsd(lig, t["ref_lig"], t["perms_t"])
            plain, _ = LA.pose_rmsd(lig, t["ref_lig"], t["ident"])
            c = LA.pose_contacts(lig, t["lig_r"], self._receptor(t, apos), t["rec_r"], t["ref_centroid"], self.overlap)
            sc = None
            if apos is not None and t["sc_rows"] is not None:
                sc, _ = LA.pose_rmsd(apos, t["sc_ref"], t["sc_ident"], sel=t["sc_rows"])
            return PoseMetrics(rmsd, plain, best, c[:, 3].contiguous(), c[:, 1].contiguous(), c[:, 2].contiguous(), c[:, 0].to(torch.int32),
                               sc, self.symmetry_corrected)

    def contact_tables(self, on_device: bool, atom_pos: Optional[torch.Tensor] = None):
        """(lig_radii [n], receptor coordinates [m, 3] or [S, m, 3], rec_radii [m]) that the contacts pass uses, on the evaluator's
        device (on_device) or on the host: the van der Waals radii of the ligand, the receptor of `receptor=` - or, for a graph
        receptor and a given atom_pos [S, n_a, 3], each sample's own atom positions - and its radii (negative: a hydrogen)."""
        t = self._dev if on_device else self._cpu
        return t["lig_r"], self._receptor(t, atom_pos), t["rec_r"]

    def contacts(self, lig_pos: torch.Tensor, atom_pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[S, 4] fp32 = clashes, min_cross, min_self, centroid of the poses alone (the contacts pass of `evaluate`, without the RMSDs),
        on the poses' device."""
        self._check_lig(lig_pos)
        lig = lig_pos.float().contiguous()
        apos = None if atom_pos is None else atom_pos.float().contiguous()
        if lig.is_cuda:
            from . import launch as LA
            t = self._dev
            with torch.cuda.device(lig.device):
                return LA.pose_contacts(lig, t["lig_r"], self._receptor(t, apos), t["rec_r"], t["ref_centroid"], self.overlap)
        t = self._cpu
        return _contacts_torch(lig, t["lig_r"], self._receptor(t, apos), t["rec_r"], t["ref_centroid"], self.overlap)

    def _check_lig(self, lig_pos):
        check_poses(self.n, self.n_a, self.device, lig_pos, None, "evaluator")

    def pairwise_rmsd(self, lig_pos: torch.Tensor) -> torch.Tensor:
        """lig_pos [S, n, 3] -> [S, S] symmetry-corrected RMSD of every pair of poses (no centring, no alignment, the minimum over
        the automorphisms - the identity alone when their search overflowed), on the poses' device: ddp_pose_pairwise_rmsd for
        device tensors, `_pairwise_torch` for CPU tensors."""
        self._check_lig(lig_pos)
        if lig_pos.is_cuda:
            from . import launch as LA
            with torch.cuda.device(lig_pos.device):
                return LA.pose_pairwise_rmsd(lig_pos.float().contiguous(), self._dev["perms_t"])
        return _pairwise_torch(lig_pos.float(), self._cpu["perms"])

    def cluster(self, lig_pos: torch.Tensor, confidence: Optional[torch.Tensor] = None, cutoff: float = 2.0) -> PoseClusters:
        """Binding modes of the poses: greedy leader clustering on `pairwise_rmsd`, walking the poses by descending confidence ([S],
        or the first column of [S, k]; None: in the order given).  Results on the poses' device."""
        dist = self.pairwise_rmsd(lig_pos)
        S = dist.shape[0]
        order = None
        if confidence is not None:
            key = confidence[:, 0] if confidence.dim() == 2 else confidence
            if key.shape != (S,):
                raise ValueError(f"confidence: expected [{S}] or [{S}, k], got {tuple(confidence.shape)}")
            order = torch.argsort(key.to(dist.device), descending=True).to(torch.int32)
        if dist.is_cuda:
            from . import launch as LA
            with torch.cuda.device(dist.device):
                labels, reps, sizes, _ = LA.pose_cluster(dist, order, cutoff)
        else:
            labels, reps, sizes, _ = _cluster_torch(dist, order, cutoff)
        has = labels >= 0
        rep_of = reps.long()[labels.long().clamp(min=0)].clamp(min=0)
        to_rep = torch.where(has, dist[rep_of, torch.arange(S, device=dist.device)], torch.full_like(dist[:, 0], float("nan"))) \
            if S else dist.new_empty(0)
        return PoseClusters(dist, labels, reps, sizes, to_rep, self.symmetry_corrected)


# ---------------------------------------------------------------------------------------------- summary over complexes
def _pct(mask) -> float:
    return round(float(100.0 * np.mean(mask)), 2) if np.size(mask) else float("nan")


def _stack(ms: Sequence[PoseMetrics], name) -> np.ndarray:
    return np.stack([getattr(m, name).detach().cpu().double().numpy() for m in ms])


def summarize(per_complex_metrics: Sequence[PoseMetrics]) -> Dict[str, float]:
    """The percentages of evaluate_files.py:261-340 over complexes whose samples are RANKED (best first), all with the same sample
    count: top-1 rows use sample 0, top-5 / top-10 rows the best RMSD among the first 5 / 10, the other rows every sample."""
    ms = list(per_complex_metrics)
    if not ms:
        return {}
    rmsds, cent = _stack(ms, "rmsd"), _stack(ms, "centroid")
    cross, self_d, clashes = _stack(ms, "min_cross"), _stack(ms, "min_self"), _stack(ms, "clashes")
    top1 = rmsds[:, 0]
    out = {
        "steric_clash_fraction": _pct(cross < 0.4), "self_intersect_fraction": _pct(self_d < 0.4),
        "top1_mean_rmsd": round(float(top1.mean()), 2), "top1_rmsds_below_2": _pct(top1 < 2), "top1_rmsds_below_5": _pct(top1 < 5),
        "mean_rmsd": round(float(rmsds.mean()), 2), "rmsds_below_2": _pct(rmsds < 2), "rmsds_below_5": _pct(rmsds < 5),
        "mean_centroid": round(float(cent[:, 0].mean()), 2), "centroid_below_2": _pct(cent[:, 0] < 2),
        "centroid_below_5": _pct(cent[:, 0] < 5),
    }
    for q in (25, 50, 75):
        out[f"top1_rmsds_percentile_{q}"] = round(float(np.percentile(top1, q)), 2)
        out[f"rmsds_percentile_{q}"] = round(float(np.percentile(rmsds, q)), 2)
        out[f"centroid_percentile_{q}"] = round(float(np.percentile(cent[:, 0], q)), 2)
    c1 = clashes[:, 0]
    out["top1_rec_lig_steric_clashes_fraction"] = _pct(c1 > 0)
    out["top1_rec_lig_steric_clashes_mean"] = round(float(c1.mean()), 2)
    rows = np.arange(rmsds.shape[0])
    for k in (5, 10):
        first = np.argsort(rmsds[:, :k], axis=1, kind="stable")[:, 0]
        tk, ck = rmsds[rows, first], cent[rows, first]
        out.update({f"top{k}_steric_clash_fraction": _pct(cross[rows, first] < 0.4),
                    f"top{k}_self_intersect_fraction": _pct(self_d[rows, first] < 0.4),
                    f"top{k}_rmsds_below_2": _pct(tk < 2), f"top{k}_rmsds_below_5": _pct(tk < 5),
                    f"top{k}_centroid_below_2": _pct(ck < 2), f"top{k}_centroid_below_5": _pct(ck < 5)})
        for q in (25, 50, 75):
            out[f"top{k}_rmsds_percentile_{q}"] = round(float(np.percentile(tk, q)), 2)
            out[f"top{k}_centroid_percentile_{q}"] = round(float(np.percentile(ck, q)), 2)
    if all(m.sc_rmsd is not None for m in ms):
        sc = _stack(ms, "sc_rmsd")
        out["mean_sidechain_rmsd"] = round(float(sc.mean()), 2)
        out["top1_mean_sidechain_rmsd"] = round(float(sc[:, 0].mean()), 2)
        for thr in (0.25, 0.5, 1, 2):
            out[f"sidechain_rmsds_below_{thr}"] = _pct(sc < thr)
            out[f"top1_sidechain_rmsds_below_{thr}"] = _pct(sc[:, 0] < thr)
        for q in (25, 50, 75):
            out[f"sidechain_rmsds_percentile_{q}"] = round(float(np.percentile(sc, q)), 2)
            out[f"top1_sidechain_rmsds_percentile_{q}"] = round(float(np.percentile(sc[:, 0], q)), 2)
    return out
