"""File output of a docking run: ranked ligand poses as SDF, the receptor with moved side chains and reverse-process trajectories as
PDB (reference inference.py:146-165,212-280, utils/visualise.py).  Host code without rdkit / Biopython; it reads what `inputs`
parses, and the formats are those of the reference's files:

- `write_sdf`: one V2000 record of the heavy-atom molecule (`inputs.remove_hs`, graph node order = the ligand nodes), name line
  from the input record, coordinates `%10.4f`, the input's bond orders, `M  CHG` for charged atoms (rdkit's MolToMolBlock layout).
- `write_ligand_trajectory`: one MODEL / ENDMDL block per frame with HETATM records (residue UNL 1, element symbols) and the
  CONECT records in the first model only, as the reference's PDBFile.write.
- `write_receptor`: the ATOM / HETATM records of the input's first model in the input's order, hydrogens dropped under remove_hs,
  of alternate locations the one `inputs.parse_pdb` keeps, the moving side-chain atoms' coordinates (columns 31-54) rewritten and
  every other line byte for byte the input's.  Deviation: the reference (SidechainPDBFile on a Bio.PDB structure) also re-sorts the
  atoms inside each residue by its SORTING_DICT; here the input's order is kept.

Coordinates handed to the writers are pocket-centred (the graph's frame); `original_center` is added on the way out."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import inputs as I


def _np(x) -> np.ndarray:
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


def _center(original_center) -> np.ndarray:
    return _np(original_center).reshape(1, 3) if original_center is not None else np.zeros((1, 3))


def sdf_name(sdf_text: str) -> str:
    """Name line of the first record."""
    return sdf_text.splitlines()[0] if sdf_text else ""


def heavy_molecule(sdf_text: str) -> I.Molecule:
    """The molecule the ligand nodes were built from (inputs.ligand_graph with remove_hs)."""
    return I.remove_hs(I.parse_sdf(sdf_text))[0]


# ---------------------------------------------------------------------------------------------- SDF
def sdf_block(mol: I.Molecule, pos, name: str = "") -> str:
    """One V2000 record (ending in `$$$$`) of `mol` at `pos` [n_atoms, 3] (absolute coordinates)."""
    pos = _np(pos).reshape(-1, 3)
    if pos.shape[0] != len(mol.elements):
        raise ValueError(f"{pos.shape[0]} coordinates for {len(mol.elements)} atoms")
    if len(mol.elements) > 999 or len(mol.bonds) > 999:
        raise ValueError("V2000 holds at most 999 atoms and bonds")
    out = [name, "     DDPAMD          3D", "",
           f"{len(mol.elements):3d}{len(mol.bonds):3d}  0  0  0  0  0  0  0  0999 V2000"]
    for (x, y, z), e in zip(pos, mol.elements):
        out.append(f"{x:10.4f}{y:10.4f}{z:10.4f} {e:<3} 0  0  0  0  0  0  0  0  0  0  0  0")
    for a, b, o in mol.bonds:
        out.append(f"{a + 1:3d}{b + 1:3d}{o:3d}  0")
    charged = [(i + 1, c) for i, c in enumerate(mol.charges) if c]
    for k in range(0, len(charged), 8):
        part = charged[k:k + 8]
        out.append(f"M  CHG{len(part):3d}" + "".join(f" {i:3d} {c:3d}" for i, c in part))
    out += ["M  END", "$$$$"]
    return "\n".join(out) + "\n"


def write_sdf(path: str, mol: I.Molecule, pos, name: str = "", original_center=None) -> str:
    """`pos` pocket-centred [n_atoms, 3]; the file gets pos + original_center."""
    with open(path, "w") as f:
        f.write(sdf_block(mol, _np(pos).reshape(-1, 3) + _center(original_center), name))
    return path


# ---------------------------------------------------------------------------------------------- ligand trajectory
def _pdb_atom_names(elements: Sequence[str]) -> List[str]:
    """rdkit's MolToPDBBlock naming: element + running number per element, one-letter elements from column 14."""
    seen: Dict[str, int] = {}
    names = []
    for e in elements:
        sym = e.upper()
        seen[sym] = seen.get(sym, 0) + 1
        nm = f"{sym}{seen[sym]}"
        names.append((" " + nm if len(sym) == 1 and len(nm) < 4 else nm)[:4].ljust(4))
    return names


def ligand_pdb_model(mol: I.Molecule, pos, conect: bool) -> List[str]:
    """HETATM records (+ CONECT) of one frame, absolute coordinates."""
    pos = _np(pos).reshape(-1, 3)
    names = _pdb_atom_names(mol.elements)
    out = []
    for i, ((x, y, z), e) in enumerate(zip(pos, mol.elements)):
        out.append(f"HETATM{i + 1:5d} {names[i]} UNL     1    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00          {e.upper():>2}  ")
    if conect:
        nbr: List[List[int]] = [[] for _ in mol.elements]
        for a, b, _ in mol.bonds:
            nbr[a].append(b)
            nbr[b].append(a)
        for i, js in enumerate(nbr):
            for k in range(0, len(js), 4):
                out.append(f"CONECT{i + 1:5d}" + "".join(f"{j + 1:5d}" for j in sorted(js)[k:k + 4]))
    return out


def write_ligand_trajectory(path: str, mol: I.Molecule, frames, original_center=None) -> str:
    """One MODEL per frame; `frames` [F, n_atoms, 3] pocket-centred (ligand_frames gives the reference's sequence)."""
    c = _center(original_center)
    out = []
    for k, pos in enumerate(frames):
        out.append(f"MODEL     {k + 1:4d}")
        out += ligand_pdb_model(mol, _np(pos).reshape(-1, 3) + c, conect=k == 0)
        out.append("ENDMDL")
    out.append("END")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return path


def ligand_frames(input_pos, traj) -> list:
    """The reference's frame order (inference.py:153-158, utils/sampling.py): input pose, input pose, then the trajectory
    (slot 0 = randomised pose, slot t + 1 = after step t): n_slots + 2 frames, pocket-centred."""
    return [input_pos, input_pos] + list(traj)


# ---------------------------------------------------------------------------------------------- receptor
def _kept_records(pdb_text: str, remove_hs: bool):
    """(lines, kept line numbers in input order, {(chain, hetflag, resseq, icode, name): line number}) over the ATOM / HETATM
    records of the first model, alternate locations resolved as inputs.parse_pdb resolves them (highest occupancy, first on ties)."""
    lines = pdb_text.splitlines()
    best: Dict[Tuple, Tuple[int, float]] = {}
    for k, ln in enumerate(lines):
        rec = ln[:6]
        if rec.startswith("ENDMDL"):
            break
        if rec not in ("ATOM  ", "HETATM"):
            continue
        resname, chain, altloc = ln[17:20].strip(), ln[21], ln[16]
        hetflag = " " if rec == "ATOM  " else ("W" if resname in ("HOH", "WAT") else "H_" + resname)
        key = (chain, hetflag, int(ln[22:26]), ln[26], ln[12:16].strip())
        try:
            occ = float(ln[54:60])
        except ValueError:
            occ = 1.0
        old = best.get(key)
        if old is None or (altloc != " " and occ > old[1]):
            best[key] = (k, occ)
    rows = {key: k for key, (k, _) in best.items()}
    kept = sorted(rows.values())
    if remove_hs:
        def element(ln):
            e = ln[76:78].strip().upper() if len(ln) >= 78 else ""
            return e or I._element_from_name(ln[12:16])
        kept = [k for k in kept if element(lines[k]) != "H"]
    return lines, kept, rows


def receptor_pdb(pdb_text: str, flex_atom_records: Dict[int, Tuple], moving: Sequence[int], frames, original_center=None,
                 remove_hs: bool = True) -> str:
    """Text of `write_receptor`.  moving [n_moving] atom node indices (sorted unique flexResidues.subcomponents); frames: a list of
    [n_moving, 3] pocket-centred positions, or None for a frame at the input coordinates."""
    lines, kept, rows = _kept_records(pdb_text, remove_hs)
    moving = [int(m) for m in moving]
    try:
        line_of = [rows[flex_atom_records[m]] for m in moving]
    except KeyError as e:
        raise ValueError(f"moving atom {e} has no PDB record") from None
    c = _center(original_center)
    multi = len(frames) > 1
    out = []
    for f, pos in enumerate(frames):
        new = {}
        if pos is not None:
            p = _np(pos).reshape(-1, 3) + c
            if p.shape[0] != len(moving):
                raise ValueError(f"{p.shape[0]} positions for {len(moving)} moving atoms")
            for k, (x, y, z) in zip(line_of, p):
                ln = lines[k]
                new[k] = ln[:30] + f"{x:8.3f}{y:8.3f}{z:8.3f}" + ln[54:]
        if multi:
            out.append(f"MODEL     {f + 1:4d}")
        out += [new.get(k, lines[k]) for k in kept]
        if multi:
            out.append("ENDMDL")
    out.append("END")
    return "\n".join(out) + "\n"


def write_receptor(path: str, pdb_text: str, graph, frames, remove_hs: bool = True) -> str:
    """The input receptor with the moving side-chain atoms of `graph` (inputs.build_complex_graph with flexible side chains) at
    `frames` (see receptor_pdb; one frame: no MODEL records)."""
    text = receptor_pdb(pdb_text, graph.flex_atom_records, moving_atoms(graph).tolist(), frames, getattr(graph, "original_center", None), remove_hs)
    with open(path, "w") as f:
        f.write(text)
    return path


def moving_atoms(graph) -> torch.Tensor:
    """Sorted unique flexResidues.subcomponents: the atom nodes side-chain torsions move (Sampler.moving_atoms)."""
    return torch.unique(torch.as_tensor(graph["flexResidues"].subcomponents).cpu())


# ---------------------------------------------------------------------------------------------- binding modes
MODES_COLUMNS = ["rank", "sample", "confidence", "mode", "is_representative", "mode_size", "rmsd_to_representative"]


def write_modes_csv(path: str, clusters, confidence=None, order=None) -> str:
    """modes.csv of one complex: one row per pose in RANKED order (evaluation.PoseClusters of the ranked poses).  rank counts from 1,
    sample is the pose's index before ranking (order [N]; None: rank - 1), confidence is empty without a confidence model; mode counts
    from 0 in the rank order of the representatives, is_representative is 0 / 1."""
    import csv
    c = clusters.cpu()
    labels, reps, sizes = c.labels.tolist(), c.representatives.tolist(), c.sizes.tolist()
    to_rep = c.rmsd_to_representative.tolist()
    conf = None
    if confidence is not None:
        conf = _np(confidence)
        conf = conf[:, 0] if conf.ndim == 2 else conf
    sample = list(range(len(labels))) if order is None else [int(v) for v in _np(order).reshape(-1)]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(MODES_COLUMNS)
        for k, m in enumerate(labels):
            w.writerow([k + 1, sample[k], "" if conf is None else f"{float(conf[k]):.4f}", m, int(m >= 0 and reps[m] == k),
                        sizes[m] if m >= 0 else 0, f"{to_rep[k]:.4f}"])
    return path


# ---------------------------------------------------------------------------------------------- clash relief
CLASHES_COLUMNS = ["rank", "sample", "clashes_before", "clashes_after", "energy_before", "energy_after", "rmsd_moved", "accepted_steps"]


def write_clashes_csv(path: str, refine, order=None) -> str:
    """clashes.csv of one complex: one row per pose in RANKED order (refine.RefineResult of the ranked poses).  rank counts from 1,
    sample is the pose's index before ranking (order [N]; None: rank - 1); the energies are the total E of refine.py before and after
    (clash terms + restraint), rmsd_moved in angstrom, accepted_steps the accepted trials of the line search."""
    import csv
    r = refine.cpu()
    sample = list(range(r.lig_pos.shape[0])) if order is None else [int(v) for v in _np(order).reshape(-1)]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CLASHES_COLUMNS)
        for k in range(r.lig_pos.shape[0]):
            w.writerow([k + 1, sample[k], int(r.clashes_before[k]), int(r.clashes_after[k]), f"{float(r.energy_before[k, 3]):.6g}",
                        f"{float(r.energy_after[k, 3]):.6g}", f"{float(r.rmsd_moved[k]):.4f}", int(r.accepted[k])])
    return path


# ---------------------------------------------------------------------------------------------- physics score
SCORES_COLUMNS = ["rank", "sample", "confidence", "total", "inter", "intra", "gauss", "repulsion", "hydrophobic", "hbond"]


def write_scores_csv(path: str, scores, confidence=None, order=None, resolved=None) -> str:
    """scores.csv of one complex: one row per pose in RANKED order (scoring.PoseScores of the ranked poses).  rank counts from 1, sample
    is the pose's index before ranking (order [N]; None: rank - 1), confidence is empty without a confidence model; total, inter and
    intra are the Vinardo-form energies of scoring.py (lower is better), gauss ... hbond the unweighted sums over the ligand-receptor
    pairs.  resolved (PoseScores of the poses after clash relief): one more column, total_resolved."""
    import csv
    sc = scores.cpu()
    N = sc.total.shape[0]
    conf = None
    if confidence is not None:
        conf = _np(confidence)
        conf = conf[:, 0] if conf.ndim == 2 else conf
    sample = list(range(N)) if order is None else [int(v) for v in _np(order).reshape(-1)]
    res = None if resolved is None else resolved.cpu()
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SCORES_COLUMNS + (["total_resolved"] if res is not None else []))
        for k in range(N):
            w.writerow([k + 1, sample[k], "" if conf is None else f"{float(conf[k]):.4f}", f"{float(sc.total[k]):.6g}",
                        f"{float(sc.inter[k]):.6g}", f"{float(sc.intra[k]):.6g}"] + [f"{float(v):.6g}" for v in sc.terms[k]]
                       + ([f"{float(res.total[k]):.6g}"] if res is not None else []))
    return path


# ---------------------------------------------------------------------------------------------- minimisation in the physics score
MINIMIZED_COLUMNS = ["rank", "sample", "total_before", "total_after", "energy_before", "energy_after", "inter_after", "intra_after",
                     "restraint_after", "rmsd_moved", "accepted_steps"]


def write_minimized_csv(path: str, minimized, order=None) -> str:
    """minimized.csv of one complex: one row per pose in RANKED order (minimize.MinimizeResult of the ranked poses).  rank counts from
    1, sample is the pose's index before ranking (order [N]; None: rank - 1); total_* are scoring.PoseScores.total of the pose before and
    after (comparable with scores.csv), energy_* the minimised E = inter + intra + restraint term of minimize.py, rmsd_moved in
    angstrom, accepted_steps the accepted trials of the line search.  A minimize_flex.FlexMinimizeResult (energies [N, 6]): the same
    columns, energy_* the joint E of minimize_flex.py, restraint_after the ligand's restraint term."""
    import csv
    r = minimized.cpu()
    e_col, rest_col = (5, 3) if r.energy_after.shape[1] == 6 else (3, 2)
    sample = list(range(r.lig_pos.shape[0])) if order is None else [int(v) for v in _np(order).reshape(-1)]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(MINIMIZED_COLUMNS)
        for k in range(r.lig_pos.shape[0]):
            w.writerow([k + 1, sample[k], f"{float(r.scores_before.total[k]):.6g}", f"{float(r.scores_after.total[k]):.6g}",
                        f"{float(r.energy_before[k, e_col]):.6g}", f"{float(r.energy_after[k, e_col]):.6g}", f"{float(r.energy_after[k, 0]):.6g}",
                        f"{float(r.energy_after[k, 1]):.6g}", f"{float(r.energy_after[k, rest_col]):.6g}", f"{float(r.rmsd_moved[k]):.4f}",
                        int(r.accepted[k])])
    return path


# ---------------------------------------------------------------------------------------------- search in the physics score
SEARCHED_COLUMNS = ["rank", "sample", "total_before", "total_after", "energy_before", "energy_minimized", "energy_after", "best_replica",
                    "best_cycle", "moves", "rmsd_moved"]


def write_searched_csv(path: str, searched, order=None) -> str:
    """searched.csv of one complex: one row per pose in RANKED order (search.SearchResult of the ranked poses).  rank and sample as
    minimized.csv; total_* are scoring.PoseScores.total of the pose before and after (comparable with scores.csv); energy_* the E of
    search.py of the sampled pose, after the plain descent of replica 0 and of the result; best_replica and best_cycle say which chain
    found the result and when (-1: the sampled pose itself), moves counts that chain's Metropolis moves, rmsd_moved is in angstrom.  A
    search_flex.FlexSearchResult (energies [N, 6]): the same columns, energy_* the joint E of search_flex.py."""
    import csv
    r = searched.cpu()
    e = r.energy_after.shape[1] - 1            # the column of E: 3, or 5 for the joint energy
    sample = list(range(r.lig_pos.shape[0])) if order is None else [int(v) for v in _np(order).reshape(-1)]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SEARCHED_COLUMNS)
        for k in range(r.lig_pos.shape[0]):
            w.writerow([k + 1, sample[k], f"{float(r.scores_before.total[k]):.6g}", f"{float(r.scores_after.total[k]):.6g}",
                        f"{float(r.energy_before[k, e]):.6g}", f"{float(r.energy_minimized[k, e]):.6g}", f"{float(r.energy_after[k, e]):.6g}",
                        int(r.replica[k]), int(r.cycle[k]), int(r.moves[k]), f"{float(r.rmsd_moved[k]):.4f}"])
    return path


MINIMIZED_SIDECHAINS_COLUMNS = ["rank", "sample", "sc_before", "sc_after", "sidechain_restraint_after", "sidechain_rmsd_moved"]


def write_minimized_sidechains_csv(path: str, minimized, order=None) -> str:
    """minimized_sidechains.csv of one complex whose side chains were minimised with the ligand (minimize_flex.FlexMinimizeResult of
    the ranked poses): one row per pose in RANKED order, rank and sample as minimized.csv; sc_* the side chains' own pair energy sc(y)
    of minimize_flex.py before and after, sidechain_restraint_after their restraint term, sidechain_rmsd_moved the RMSD over the
    moving atoms in angstrom."""
    import csv
    r = minimized.cpu()
    sample = list(range(r.lig_pos.shape[0])) if order is None else [int(v) for v in _np(order).reshape(-1)]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(MINIMIZED_SIDECHAINS_COLUMNS)
        for k in range(r.lig_pos.shape[0]):
            w.writerow([k + 1, sample[k], f"{float(r.energy_before[k, 2]):.6g}", f"{float(r.energy_after[k, 2]):.6g}",
                        f"{float(r.energy_after[k, 4]):.6g}", f"{float(r.sidechain_rmsd_moved[k]):.4f}"])
    return path


def write_searched_sidechains_csv(path: str, searched, order=None) -> str:
    """searched_sidechains.csv of one complex whose side chains were searched with the ligand (search_flex.FlexSearchResult of the ranked
    poses): the columns of minimized_sidechains.csv, one row per pose in RANKED order; sc_* the side chains' own pair energy sc(y) of the
    sampled state and of the result, sidechain_restraint_after their restraint term, sidechain_rmsd_moved the RMSD over the moving atoms
    in angstrom."""
    return write_minimized_sidechains_csv(path, searched, order)


# ---------------------------------------------------------------------------------------------- interaction profile
INTERACTIONS_COLUMNS = ["rank", "sample", "residue", "gauss", "repulsion", "hydrophobic", "hbond", "energy", "d_min", "contact",
                        "hydrophobic_bit", "hbond_bit"]
INTERACTION_SUMMARY_COLUMNS = ["residue", "contact_freq", "hydrophobic_freq", "hbond_freq", "mean_energy"]
INTERACTION_SIMILARITY_COLUMNS = ["rank", "sample", "tanimoto_to_rank1"]
INTERACTION_REFERENCE_COLUMNS = ["tanimoto_to_reference", "recovery_of_reference"]


def write_interactions_csv(path: str, interactions, order=None) -> str:
    """interactions.csv of one complex (interactions.InteractionProfile of the ranked poses): one row per pose and residue that have at
    least one atom pair inside the cutoff (pairs > 0), poses in RANKED order, residues in receptor order.  rank counts from 1, sample is
    the pose's index before ranking (order [N]; None: rank - 1); gauss ... hbond are the unweighted sums over the residue's pairs,
    energy the residue's share of the Vinardo-form `inter`, d_min the closest centre distance in angstrom, the last three the bits."""
    import csv
    p = interactions.cpu()
    N = p.bits.shape[0]
    sample = list(range(N)) if order is None else [int(v) for v in _np(order).reshape(-1)]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(INTERACTIONS_COLUMNS)
        for k in range(N):
            for r in torch.nonzero(p.pairs[k] > 0).flatten().tolist():
                b = int(p.bits[k, r])
                w.writerow([k + 1, sample[k], p.labels[r]] + [f"{float(v):.6g}" for v in p.terms[k, r]]
                           + [f"{float(p.energy[k, r]):.6g}", f"{float(p.d_min[k, r]):.4f}", b & 1, (b >> 1) & 1, (b >> 2) & 1])
    return path


def write_interaction_summary_csv(path: str, interactions) -> str:
    """interaction_summary.csv of one complex: one row per residue that any pose reaches (pairs > 0), in receptor order: the share of
    the poses with each bit set and the mean of the residue's energy over the poses (a poisoned pose, NaN, is left out of the mean)."""
    import csv
    p = interactions.cpu()
    freq = p.frequency()
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(INTERACTION_SUMMARY_COLUMNS)
        for r in torch.nonzero((p.pairs > 0).any(0)).flatten().tolist():
            w.writerow([p.labels[r]] + [f"{float(v):.4f}" for v in freq[r]] + [f"{float(torch.nanmean(p.energy[:, r])):.6g}"])
    return path


def write_interaction_similarity_csv(path: str, interactions, order=None, reference=None) -> str:
    """interaction_similarity.csv of one complex: one row per pose in RANKED order with the Tanimoto similarity of its interaction bits
    to those of the pose ranked first.  reference (the InteractionProfile of the known pose, one row): two more columns, the Tanimoto
    similarity to the known pose's bits and the share of them that the pose recovers (empty where the known pose sets no bit)."""
    import csv
    p = interactions.cpu()
    N = p.bits.shape[0]
    sample = list(range(N)) if order is None else [int(v) for v in _np(order).reshape(-1)]
    first = p.tanimoto_to(p.bits[0]) if N else []
    to_ref = rec = None
    if reference is not None:
        rb = reference.cpu().bits[0]
        to_ref, rec = p.tanimoto_to(rb), p.recovery(rb)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(INTERACTION_SIMILARITY_COLUMNS + (INTERACTION_REFERENCE_COLUMNS if reference is not None else []))
        for k in range(N):
            row = [k + 1, sample[k], f"{float(first[k]):.4f}"]
            if reference is not None:
                row += [f"{float(to_ref[k]):.4f}", "" if bool(torch.isnan(rec[k])) else f"{float(rec[k]):.4f}"]
            w.writerow(row)
    return path


# ---------------------------------------------------------------------------------------------- pockets
POCKETS_COLUMNS = ["pocket", "score", "size", "center_x", "center_y", "center_z", "ca_center_x", "ca_center_y", "ca_center_z", "docked"]


def write_pockets_csv(path: str, pockets, docked: int = 1) -> str:
    """pockets.csv of one complex docked without a given centre (pockets.find_pockets, best first): one line per pocket FOUND, pocket
    counts from 1, the centres in the input frame, docked = 1 for the first `docked` pockets (the ones the run docked into)."""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(POCKETS_COLUMNS)
        for k, p in enumerate(pockets):
            w.writerow([k + 1, int(p.score), int(p.size)] + [f"{float(v):.4f}" for v in p.center] + [f"{float(v):.4f}" for v in p.ca_center]
                       + [int(k < docked)])
    return path


# ---------------------------------------------------------------------------------------------- one complex
def complex_dir(out_dir: str, index: int, name: str) -> str:
    """reference inference.py:136."""
    return os.path.join(out_dir, f'index{index}___{name.replace("/", "-")}')


def write_complex(write_dir: str, sdf_text: str, pdb_text: Optional[str], graph, ligand_pos, confidence=None, atom_pos=None,
                  lig_traj=None, atom_traj=None, remove_hs: bool = True, clusters=None, order=None, refine=None, pockets=None,
                  pockets_docked: int = 1, scores=None, refined_scores=None, minimized=None, interactions=None,
                  interaction_reference=None, searched=None) -> List[str]:
    """Files of one complex (reference inference.py:240-280), all inputs in RANKED order, pocket-centred:
    ligand_pos [N, n_lig, 3]; confidence [N] or [N, k] (first column) or None; atom_pos [N, n_atoms, 3] of a flexible run or None;
    lig_traj [N, n_slots, n_lig, 3] / atom_traj [N, n_slots, n_moving, 3] with save_visualisation.  Returns the paths written.

    With a confidence model: rank1.sdf and rank{k}_confidence{c:.2f}.sdf; without one rank{k}.sdf (the reference fails there).
    Flexible: rank1_protein.pdb and rank{k}_confidence{c:.2f}_protein.pdb (rank{k}_protein.pdb).  Trajectories:
    rank{k}_reverseprocess.pdb and rank{k}_reverseprocess_protein.pdb, each of the ranked sample itself (the reference indexes the
    side-chain trajectories by rank instead of by sample, inference.py:276-279).
    clusters (evaluation.PoseClusters of the ranked poses; order [N]: the sample index of each rank): also modes.csv.
    refine (refine.RefineResult of the ranked poses): also rank{k}_resolved.sdf, the pose after clash relief, and clashes.csv.
    pockets (pockets.find_pockets of the protein, when the centre came from there): also pockets.csv.
    scores (scoring.PoseScores of the ranked poses; refined_scores: of the poses after clash relief): also scores.csv.
    minimized (minimize.MinimizeResult of the ranked poses): also rank{k}_minimized.sdf, the pose after the minimisation in the physics
    score, and minimized.csv; a minimize_flex.FlexMinimizeResult: also rank{k}_minimized_protein.pdb, the receptor with the side chains
    the pose was minimised with (write_receptor), and minimized_sidechains.csv.
    interactions (interactions.InteractionProfile of the ranked poses; interaction_reference: of the known pose): also interactions.csv,
    interaction_summary.csv and interaction_similarity.csv.
    searched (search.SearchResult of the ranked poses): also rank{k}_searched.sdf, the pose after the search in the physics score, and
    searched.csv; a search_flex.FlexSearchResult: also rank{k}_searched_protein.pdb, the receptor with the side chains the pose was
    searched with (write_receptor), and searched_sidechains.csv."""
    os.makedirs(write_dir, exist_ok=True)
    mol = heavy_molecule(sdf_text)
    name, oc = sdf_name(sdf_text), getattr(graph, "original_center", None)
    conf = None
    if confidence is not None:
        conf = _np(confidence)
        conf = conf[:, 0] if conf.ndim == 2 else conf
    tag = (lambda k: f"rank{k + 1}_confidence{conf[k]:.2f}") if conf is not None else (lambda k: f"rank{k + 1}")
    moving = moving_atoms(graph).tolist() if atom_pos is not None or atom_traj is not None else None
    written = []

    def put(path):
        written.append(path)
        return path

    for k in range(ligand_pos.shape[0]):
        if k == 0 and conf is not None:
            write_sdf(put(os.path.join(write_dir, "rank1.sdf")), mol, ligand_pos[k], name, oc)
        write_sdf(put(os.path.join(write_dir, tag(k) + ".sdf")), mol, ligand_pos[k], name, oc)
    if atom_pos is not None:
        for k in range(atom_pos.shape[0]):
            text = receptor_pdb(pdb_text, graph.flex_atom_records, moving, [_np(atom_pos[k])[moving]], oc, remove_hs)
            for fn in (["rank1_protein.pdb"] if k == 0 and conf is not None else []) + [tag(k) + "_protein.pdb"]:
                with open(put(os.path.join(write_dir, fn)), "w") as f:
                    f.write(text)
    if lig_traj is not None:
        start = graph["ligand"].pos
        for k in range(lig_traj.shape[0]):
            write_ligand_trajectory(put(os.path.join(write_dir, f"rank{k + 1}_reverseprocess.pdb")), mol,
                                    ligand_frames(start, lig_traj[k]), oc)
    if atom_traj is not None:
        for k in range(atom_traj.shape[0]):
            frames = [None, None] + [f for f in atom_traj[k]]
            text = receptor_pdb(pdb_text, graph.flex_atom_records, moving, frames, oc, remove_hs)
            with open(put(os.path.join(write_dir, f"rank{k + 1}_reverseprocess_protein.pdb")), "w") as f:
                f.write(text)
    if clusters is not None:
        write_modes_csv(put(os.path.join(write_dir, "modes.csv")), clusters, confidence, order)
    if refine is not None:
        for k in range(refine.lig_pos.shape[0]):
            write_sdf(put(os.path.join(write_dir, f"rank{k + 1}_resolved.sdf")), mol, refine.lig_pos[k], name, oc)
        write_clashes_csv(put(os.path.join(write_dir, "clashes.csv")), refine, order)
    if pockets is not None:
        write_pockets_csv(put(os.path.join(write_dir, "pockets.csv")), pockets, pockets_docked)
    if scores is not None:
        write_scores_csv(put(os.path.join(write_dir, "scores.csv")), scores, confidence, order, refined_scores)
    if minimized is not None:
        for k in range(minimized.lig_pos.shape[0]):
            write_sdf(put(os.path.join(write_dir, f"rank{k + 1}_minimized.sdf")), mol, minimized.lig_pos[k], name, oc)
        write_minimized_csv(put(os.path.join(write_dir, "minimized.csv")), minimized, order)
        if hasattr(minimized, "atom_pos"):
            mv = moving_atoms(graph).tolist()
            for k in range(minimized.atom_pos.shape[0]):
                write_receptor(put(os.path.join(write_dir, f"rank{k + 1}_minimized_protein.pdb")), pdb_text, graph,
                               [_np(minimized.atom_pos[k])[mv]], remove_hs)
            write_minimized_sidechains_csv(put(os.path.join(write_dir, "minimized_sidechains.csv")), minimized, order)
    if searched is not None:
        for k in range(searched.lig_pos.shape[0]):
            write_sdf(put(os.path.join(write_dir, f"rank{k + 1}_searched.sdf")), mol, searched.lig_pos[k], name, oc)
        write_searched_csv(put(os.path.join(write_dir, "searched.csv")), searched, order)
        if hasattr(searched, "atom_pos"):
            mv = moving_atoms(graph).tolist()
            for k in range(searched.atom_pos.shape[0]):
                write_receptor(put(os.path.join(write_dir, f"rank{k + 1}_searched_protein.pdb")), pdb_text, graph,
                               [_np(searched.atom_pos[k])[mv]], remove_hs)
            write_searched_sidechains_csv(put(os.path.join(write_dir, "searched_sidechains.csv")), searched, order)
    if interactions is not None:
        write_interactions_csv(put(os.path.join(write_dir, "interactions.csv")), interactions, order)
        write_interaction_summary_csv(put(os.path.join(write_dir, "interaction_summary.csv")), interactions)
        write_interaction_similarity_csv(put(os.path.join(write_dir, "interaction_similarity.csv")), interactions, order,
                                         interaction_reference)
    return written
