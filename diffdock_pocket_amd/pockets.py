"""Geometric pocket finder: LIGSITE-style buriedness on a grid, so that a protein + ligand pair can be docked without a known centre.
This is the package's own method - geometry only, no learned predictor (the reference leaves the pocket centre to an outside pocket
predictor); its constants are untuned beyond the 3dpf fixture.  On a HIP device the grid work runs in csrc/ddp_pockets.hip, on the CPU
the same arithmetic in PyTorch fp32 / integer ops; grouping, ranking and the centres are NumPy on the short list of pocket points.

Definition.  Inputs: the heavy atoms of the protein's ATOM records (no waters, no HETATM - cofactors are ignored -, no hydrogens),
positions fp32, radii from assets/vdw_radii.json.  With spacing s:
  grid        (host, fp64) lo = floor((min(pos) - margin) / s) s per axis, dims = ceil((max(pos) + margin - lo) / s) + 1; point (i, j, k)
              sits at lo + (i, j, k) s and has the flat index (i ny + j) nz + k; everything outside the grid is free space.
  occupancy   occ[g] = 1 iff some atom has |x_g - x_j|^2 < (r_j + probe)^2 (strict).  fp32 with separate roundings (no FMA):
              x_g = fp32(lo) + fp32(i) fp32(s) per axis, the differences, (dx dx + dy dy) + dz dz, compared with fp32((r_j + probe)^2)
              formed in fp64 on the host - the device, torch fp32 and NumPy fp32 take the same decisions bit for bit.
  buriedness  7 lines (3 axes, 4 cube diagonals) of two opposite rays; a ray from a free point takes 1 ... floor(ray_length / (s |d|))
              grid steps along d and hits if it meets an occupied point before it leaves the grid.  bur[g] = lines with both rays
              hitting (0 ... 7; 0 at occupied points).
  pocket pts  free and bur >= min_lines.
  components  6-connectivity; a point's label is the smallest flat index of its component.
  pockets     components of at least min_points points; score = sum of bur, ranked by score descending, ties by the smaller label, the
              best max_pockets kept.  center = bur-weighted mean of the point coordinates (fp64 from integer sums); ca_center = mean of
              the C-alphas within ca_cutoff of any point of the pocket, the nearest C-alpha when there is none (the reference's own
              convention for a pocket centre, inputs.binding_pocket, with the pocket's points in the ligand's place)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .evaluation import _is_h, vdw_radius
from .inputs import PdbResidue, parse_pdb

_LINES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))


@dataclass
class PocketConfig:
    spacing: float = 1.0
    probe: float = 1.4
    ray_length: float = 10.0
    min_lines: int = 6
    min_points: int = 20
    margin: float = 2.0
    ca_cutoff: float = 5.0
    max_pockets: int = 16

    def check(self):
        if not (self.spacing > 0 and math.isfinite(self.spacing)) or self.probe < 0 or self.ray_length < 0 or self.margin < 0:
            raise ValueError("PocketConfig: spacing must be positive; probe, ray_length and margin must not be negative")
        if not 0 <= int(self.min_lines) <= 7 or self.min_points < 1 or self.max_pockets < 1:
            raise ValueError("PocketConfig: min_lines in [0, 7], min_points >= 1, max_pockets >= 1")


@dataclass
class Pocket:
    center: np.ndarray        # float64 [3], input frame: bur-weighted mean of the points
    ca_center: np.ndarray     # float64 [3]: what to pass to build_complex_graph as pocket_center
    score: int                # sum of bur over the points
    size: int                 # number of points
    points: np.ndarray        # float64 [size, 3] coordinates of the pocket's grid points, ascending flat index
    label: int = -1           # smallest flat index of the component


class PocketGrid(NamedTuple):
    lo: np.ndarray            # float64 [3]
    dims: Tuple[int, int, int]
    occ: np.ndarray           # uint8 [nx, ny, nz]
    bur: np.ndarray           # uint8 [nx, ny, nz]
    labels: np.ndarray        # int32 [nx, ny, nz], -1 outside the pocket points


# ---------------------------------------------------------------------------------------------- inputs
def protein_atoms(protein: Union[str, Sequence[PdbResidue]]):
    """(pos float32 [N, 3], radii float64 [N], ca float32 [M, 3]) of a PDB text or parsed residues: heavy atoms of ATOM records."""
    residues = parse_pdb(protein) if isinstance(protein, str) else protein
    pos, rad, ca = [], [], []
    for r in residues:
        if r.hetflag != " ":
            continue
        for a in r.atoms:
            if _is_h(a.element) or a.element.strip().upper() == "D":
                continue
            pos.append(a.coord)
            rad.append(vdw_radius(a.element))
            if a.name == "CA":
                ca.append(a.coord)
    return (np.asarray(pos, dtype=np.float32).reshape(-1, 3), np.asarray(rad, dtype=np.float64),
            np.asarray(ca, dtype=np.float32).reshape(-1, 3))


def make_grid(pos: np.ndarray, config: PocketConfig):
    """(lo float64 [3], dims (nx, ny, nz)) of the definition; raises on an empty protein or a grid of 2^31 points or more."""
    if pos.shape[0] == 0:
        raise ValueError("pocket finder: the protein has no heavy atom in its ATOM records")
    p = np.asarray(pos, dtype=np.float64)
    if not np.isfinite(p).all():
        raise ValueError("pocket finder: non-finite atom coordinate")
    s = float(config.spacing)
    lo = np.floor((p.min(0) - config.margin) / s) * s
    dims = np.ceil((p.max(0) + config.margin - lo) / s).astype(np.int64) + 1
    if int(np.prod(dims.astype(object))) >= 2 ** 31:
        raise ValueError(f"pocket finder: a grid of {tuple(int(d) for d in dims)} points is too large (spacing {s})")
    return lo, tuple(int(d) for d in dims)


def squared_reach(radii: np.ndarray, probe: float) -> np.ndarray:
    """fp32((r + probe)^2), the square formed in fp64."""
    return ((np.asarray(radii, dtype=np.float64) + float(probe)) ** 2).astype(np.float32)


def ray_steps(spacing: float, ray_length: float) -> Tuple[int, int]:
    """Grid steps of an axis ray and of a cube-diagonal ray."""
    return int(math.floor(ray_length / spacing)), int(math.floor(ray_length / (spacing * math.sqrt(3.0))))


# ---------------------------------------------------------------------------------------------- the CPU path (torch)
def occupancy_torch(pos: torch.Tensor, r2: torch.Tensor, lo, spacing: float, dims) -> torch.Tensor:
    """The occupancy of ddp_pocket_occupancy in torch fp32, atom by atom over the atom's bounding box as the kernel does it."""
    nx, ny, nz = dims
    occ = torch.zeros((nx, ny, nz), dtype=torch.bool)
    s = torch.tensor(float(spacing), dtype=torch.float32)
    lo32 = torch.as_tensor(np.asarray(lo, dtype=np.float64), dtype=torch.float32)
    axes = [lo32[d] + torch.arange(n, dtype=torch.float32) * s for d, n in enumerate(dims)]      # product, then sum: two roundings
    pos, r2 = pos.float().cpu(), r2.float().cpu()
    inv = 1.0 / float(s)
    for a in range(pos.shape[0]):
        rr = float(r2[a])
        if not rr > 0 or not bool(torch.isfinite(pos[a]).all()):
            continue
        reach = math.sqrt(rr) * inv if math.isfinite(rr) else math.inf
        sl, sq = [], []
        for d, n in enumerate(dims):
            c = (float(pos[a, d]) - float(lo32[d])) * inv
            i0 = int(min(max(math.floor(c - reach) - 2 if math.isfinite(reach) else 0, 0), n))
            i1 = int(min(max(math.ceil(c + reach) + 2 if math.isfinite(reach) else n - 1, -1), n - 1))
            sl.append(slice(i0, i1 + 1))
            diff = axes[d][i0:i1 + 1] - pos[a, d]
            sq.append(diff * diff)
        if any(q.numel() == 0 for q in sq):
            continue
        d2 = (sq[0][:, None, None] + sq[1][None, :, None]) + sq[2][None, None, :]
        occ[sl[0], sl[1], sl[2]] |= d2 < r2[a]
    return occ.to(torch.uint8)


def _shifted_any(occ_pad: torch.Tensor, pad: int, dims, d, steps: int) -> torch.Tensor:
    """hit[g] = an occupied point among g + t d, t = 1 ... steps (occ_pad: the grid padded by `pad` free points on every side)."""
    nx, ny, nz = dims
    hit = torch.zeros(dims, dtype=torch.bool)
    for t in range(1, steps + 1):
        if t > max(dims):
            break
        ox, oy, oz = pad + t * d[0], pad + t * d[1], pad + t * d[2]
        hit |= occ_pad[ox:ox + nx, oy:oy + ny, oz:oz + nz]
    return hit


def buriedness_torch(occ: torch.Tensor, spacing: float, ray_length: float, min_lines: int):
    """(bur uint8, mask int32 = bur + 1 at the pocket points, else 0) of ddp_pocket_buriedness in torch integer ops."""
    dims = tuple(occ.shape)
    n_axis, n_diag = ray_steps(spacing, ray_length)
    pad = min(max(n_axis, n_diag), max(dims))
    o = occ.cpu() != 0
    occ_pad = torch.zeros(tuple(n + 2 * pad for n in dims), dtype=torch.bool)
    occ_pad[pad:pad + dims[0], pad:pad + dims[1], pad:pad + dims[2]] = o
    bur = torch.zeros(dims, dtype=torch.int32)
    for l, d in enumerate(_LINES):
        steps = min(n_axis if l < 3 else n_diag, pad)
        bur += (_shifted_any(occ_pad, pad, dims, d, steps) & _shifted_any(occ_pad, pad, dims, tuple(-x for x in d), steps)).int()
    bur[o] = 0
    mask = torch.where(~o & (bur >= int(min_lines)), bur + 1, torch.zeros_like(bur))
    return bur.to(torch.uint8), mask


def label_torch(mask: torch.Tensor) -> torch.Tensor:
    """Labels of ddp_pocket_label in torch integer ops: minimum-label hooking over the 6-neighbour edges of the masked points with
    pointer jumping, until nothing changes."""
    dims = tuple(mask.shape)
    nx, ny, nz = dims
    m = mask.cpu() != 0
    flat = torch.nonzero(m.reshape(-1)).reshape(-1)          # ascending: compact id order = flat index order
    labels = torch.full((nx * ny * nz,), -1, dtype=torch.int64)
    if flat.numel() == 0:
        return labels.reshape(dims).int()
    compact = torch.full((nx * ny * nz,), -1, dtype=torch.int64)
    compact[flat] = torch.arange(flat.numel())
    k, j, i = flat % nz, (flat // nz) % ny, flat // (nz * ny)
    ea, eb = [], []
    for ok, step in ((k + 1 < nz, 1), (j + 1 < ny, nz), (i + 1 < nx, ny * nz)):
        src = flat[ok]
        dst = compact[src + step]
        keep = dst >= 0
        ea.append(compact[src][keep])
        eb.append(dst[keep])
    ea, eb = torch.cat(ea), torch.cat(eb)
    lab = torch.arange(flat.numel())
    while True:
        la, lb = lab[ea], lab[eb]
        lo = torch.minimum(la, lb)
        new = lab.clone()
        for idx in (la, lb, ea, eb):
            new.scatter_reduce_(0, idx, lo, reduce="amin")
        while True:
            nn = new[new]
            if torch.equal(nn, new):
                break
            new = nn
        if torch.equal(new, lab):
            break
        lab = new
    labels[flat] = flat[lab]
    return labels.reshape(dims).int()


# ---------------------------------------------------------------------------------------------- the host part, from the point list
def pockets_from_points(flat: np.ndarray, label: np.ndarray, bur: np.ndarray, lo: np.ndarray, dims, ca: np.ndarray,
                        config: PocketConfig) -> List[Pocket]:
    """Grouping, the min_points filter, the ranking and the two centres, from the compacted pocket points (flat ascending)."""
    if flat.size == 0:
        return []
    flat, label, bur = flat.astype(np.int64), label.astype(np.int64), bur.astype(np.int64)
    nx, ny, nz = dims
    ijk = np.stack([flat // (nz * ny), (flat // nz) % ny, flat % nz], 1)
    labs, inv = np.unique(label, return_inverse=True)
    size = np.bincount(inv, minlength=labs.size)
    score = np.bincount(inv, weights=bur, minlength=labs.size).astype(np.int64)
    keep = np.nonzero(size >= config.min_points)[0]
    keep = sorted(keep.tolist(), key=lambda c: (-int(score[c]), int(labs[c])))[: config.max_pockets]
    s, lo = float(config.spacing), np.asarray(lo, dtype=np.float64)
    ca64 = np.asarray(ca, dtype=np.float64).reshape(-1, 3)
    out = []
    for c in keep:
        sel = inv == c
        idx, w = ijk[sel], bur[sel]
        pts = lo[None, :] + idx.astype(np.float64) * s
        if int(score[c]) > 0:
            center = lo + s * ((idx * w[:, None]).sum(0).astype(np.float64) / float(score[c]))
        else:      # min_lines = 0 and nothing buried: the plain mean
            center = lo + s * (idx.sum(0).astype(np.float64) / float(size[c]))
        if ca64.shape[0] == 0:
            ca_center = center.copy()
        else:
            d = np.sqrt(((ca64[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
            near = (d < config.ca_cutoff).any(1)
            ca_center = ca64[near].mean(0) if near.any() else ca64[d.min(1).argmin()]
        out.append(Pocket(center=center, ca_center=ca_center, score=int(score[c]), size=int(size[c]), points=pts, label=int(labs[c])))
    return out


# ---------------------------------------------------------------------------------------------- the two grid paths
def _grid_torch(pos, r2, lo, dims, config):
    occ = occupancy_torch(torch.from_numpy(pos), torch.from_numpy(r2), lo, config.spacing, dims)
    bur, mask = buriedness_torch(occ, config.spacing, config.ray_length, config.min_lines)
    labels = label_torch(mask)
    flat = torch.nonzero(mask.reshape(-1)).reshape(-1)
    pts = (flat.numpy(), labels.reshape(-1)[flat].numpy(), bur.reshape(-1)[flat].numpy())
    return pts, (occ, bur, labels)


def _grid_hip(pos, r2, lo, dims, config, device):
    """occupancy, buriedness, labels and the compaction of the pocket points on the device; ONE synchronising copy (the count and the
    three lists in one buffer) ends the device part."""
    from . import launch as K
    n = dims[0] * dims[1] * dims[2]
    with torch.cuda.device(device):
        lo32 = np.asarray(lo, dtype=np.float64).astype(np.float32)
        occ = K.pocket_occupancy(torch.from_numpy(pos).to(device), torch.from_numpy(r2).to(device), lo32, np.float32(config.spacing), dims)
        bur, mask = K.pocket_buriedness(occ, config.spacing, config.ray_length, config.min_lines)
        labels = K.pocket_label(mask)
        buf = torch.empty(4 + 3 * n, dtype=torch.int32, device=device)     # [count, pad x 3 | flat | label | bur]: lists 16-byte aligned
        scratch = torch.empty(2 * ((n + 2047) // 2048) + 1, dtype=torch.int32, device=device)
        m1, l1 = mask.reshape(-1), labels.reshape(-1)
        K.select_jobs([K.select_job(n, m1, None, None, None, [l1, m1], [buf[4 + n:4 + 2 * n], buf[4 + 2 * n:]], buf[:1], scratch,
                                    out_idx=buf[4:4 + n], pay_add=[0, -1])])
        host = buf.cpu().numpy()
    cnt = int(host[0])
    if not 0 <= cnt <= n:
        raise RuntimeError(f"pocket finder: the device reported {cnt} pocket points on a grid of {n}")
    pts = (host[4:4 + cnt], host[4 + n:4 + n + cnt], host[4 + 2 * n:4 + 2 * n + cnt])
    return pts, (occ, bur, labels)


def find_pockets_atoms(pos: np.ndarray, radii: np.ndarray, ca: np.ndarray, device="cpu", config: Optional[PocketConfig] = None,
                       return_grid: bool = False):
    """find_pockets on explicit atoms: pos [N, 3] (fp32), radii [N], ca [M, 3] (the C-alphas, for ca_center)."""
    config = config or PocketConfig()
    config.check()
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    if radii.shape[0] != pos.shape[0]:
        raise ValueError("pocket finder: one radius per atom")
    lo, dims = make_grid(pos, config)
    r2 = squared_reach(radii, config.probe)
    dev = torch.device(device)
    if dev.type == "cuda":
        pts, grid = _grid_hip(pos, r2, lo, dims, config, dev)
    else:
        pts, grid = _grid_torch(pos, r2, lo, dims, config)
    pockets = pockets_from_points(pts[0], pts[1], pts[2], lo, dims, ca, config)
    if not return_grid:
        return pockets
    occ, bur, labels = (t.cpu().numpy() for t in grid)
    return pockets, PocketGrid(lo, dims, occ, bur, labels)


def find_pockets(protein: Union[str, Sequence[PdbResidue]], device="cpu", config: Optional[PocketConfig] = None, return_grid: bool = False):
    """Pockets of a protein (PDB text, or inputs.parse_pdb residues), best first: List[Pocket], with return_grid=True also the PocketGrid
    (lo, dims, occ, bur, labels as host arrays).  On a HIP device the grid work runs in the kernels of csrc/ddp_pockets.hip, with
    device="cpu" in torch; both give the same pockets.  Pass `pocket.ca_center` to build_complex_graph as pocket_center."""
    pos, radii, ca = protein_atoms(protein)
    return find_pockets_atoms(pos, radii, ca, device, config, return_grid)
