"""Batch driver over a `protein_ligand_csv` (BASELINE configs[3]): the loop of reference inference.py:459-493 around the
sampler, for one process per GPU.

    complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains
    (reference data/protein_ligand_example.csv; datasets/pdbbind.py:1005-1066 `load_protein_ligand_df`: rows without a
    ligand / protein are dropped, empty pocket / side-chain cells mean "not given")

Per row: the complex graph from PDB / SDF text (inputs.build_complex_graph - no rdkit / biopython), precomputed ESM rows
(`esm_embeddings`: a {complex_name: [n_residues, 1280]} mapping, or a directory of `<complex_name>.pt` / `.npy` files; the ESM
language model itself is out of scope), `samples_per_complex` poses through Sampler, the confidence
pass and the ranking of reference inference.py:212-219.

Multi-GPU: the SAMPLES of every complex are sharded over the ranks - rank r owns samples
[r*N/R, (r+1)*N/R) of the job's seeded noise stream, no collective inside the denoising loop - and the final ligand poses
and confidences are gathered once per complex (`torch.distributed.all_gather`, RCCL on the GPUs).  The reference shards
COMPLEXES over a process pool instead (inference.py:468, `np.array_split`): `shard="complexes"` does that (no collective at
all; rank r gets rows r::R... contiguous chunks as np.array_split gives them).

Only SDF ligands are read (the reference also accepts SMILES / mol2 through rdkit: out of scope, such rows are reported as
skipped, like the reference's per-complex try / except that returns 0 and goes on, inference.py:282-287)."""
from __future__ import annotations

import csv
import dataclasses
import functools
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import inputs as I
from . import outputs as O
from .diffusion import get_t_schedule
from .evaluation import PoseClusters, PoseEvaluator, PoseMetrics  # noqa: F401
from .pockets import Pocket, PocketConfig, find_pockets as _find_pockets  # noqa: F401
from .interactions import InteractionProfile, InteractionProfiler, ProfileConfig, receptor_residues  # noqa: F401
from .minimize import MinimizeConfig, MinimizeResult, PoseMinimizer  # noqa: F401
from .minimize_flex import FlexMinimizeResult, FlexPoseMinimizer  # noqa: F401
from .search import PoseSearcher, SearchConfig, SearchResult  # noqa: F401
from .search_flex import FlexPoseSearcher, FlexSearchResult  # noqa: F401
from .refine import PoseRefiner, RefineConfig, RefineResult  # noqa: F401
from .sampler import Sampler, SamplerConfig
from .scoring import PoseScorer, PoseScores, ScoreConfig, rank_order, typed_receptor  # noqa: F401


@dataclass
class ComplexResult:
    name: str
    ligand_pos: Optional[torch.Tensor] = None      # [N, n_lig, 3], pocket-centred coordinates, ranked best first
    confidence: Optional[torch.Tensor] = None      # [N] (or [N, k]), same order
    order: Optional[torch.Tensor] = None           # sample indices in ranked order
    original_center: Optional[torch.Tensor] = None
    skipped: Optional[str] = None                  # reason, if the row could not be processed
    metrics: Optional["PoseMetrics"] = None        # run_csv(evaluate=True): evaluation.PoseMetrics against the input pose, ranked order
    files: List[str] = field(default_factory=list)  # run_csv(out_dir=...): the paths written for this row
    lig_traj: Optional[torch.Tensor] = None        # save_visualisation: [N, steps + 1, n_lig, 3] reverse process, ranked order
    atom_traj: Optional[torch.Tensor] = None       # save_visualisation, flexible row: [N, steps + 1, n_moving, 3], ranked order
    clusters: Optional["PoseClusters"] = None      # run_csv(cluster_rmsd=X): evaluation.PoseClusters of the ranked poses (binding modes)
    refined_pos: Optional[torch.Tensor] = None     # run_csv(resolve_clashes=cfg): [N, n_lig, 3] the ranked poses after clash relief
    refine: Optional["RefineResult"] = None        # run_csv(resolve_clashes=cfg): refine.RefineResult of the ranked poses (host tensors)
    refined_metrics: Optional["PoseMetrics"] = None  # resolve_clashes with evaluate=True: PoseMetrics of refined_pos (`metrics` is untouched)
    pockets: Optional[List["Pocket"]] = None       # run_csv(find_pockets=cfg), row without a centre: every pocket found, best first
    scores: Optional["PoseScores"] = None          # run_csv(score_poses=cfg): scoring.PoseScores of the ranked poses (host tensors)
    refined_scores: Optional["PoseScores"] = None  # score_poses with resolve_clashes: PoseScores of refined_pos
    minimized: Optional["MinimizeResult"] = None   # run_csv(minimize_poses=cfg): minimize.MinimizeResult of the ranked poses (host tensors);
    #                                                a flexible row with cfg.sidechains: minimize_flex.FlexMinimizeResult
    minimized_pos: Optional[torch.Tensor] = None   # run_csv(minimize_poses=cfg): [N, n_lig, 3] the ranked poses after the minimisation
    searched: Optional["SearchResult"] = None      # run_csv(search_poses=cfg): search.SearchResult of the ranked poses (host tensors);
    #                                                a flexible row with cfg.sidechains: search_flex.FlexSearchResult
    searched_pos: Optional[torch.Tensor] = None    # run_csv(search_poses=cfg): [N, n_lig, 3] the ranked poses after the search
    interactions: Optional["InteractionProfile"] = None  # run_csv(interaction_profile=cfg): interactions.InteractionProfile of the ranked
    #                                                      poses (host tensors)
    interaction_reference: Optional["InteractionProfile"] = None  # interaction_profile with evaluate=True: the profile of the input pose

    def clear(self):
        """A stage of the row failed: every result goes back to its default.  What says which row it was and why it ended stays."""
        for f in dataclasses.fields(self):
            if f.name not in ("name", "skipped", "pockets", "original_center"):
                setattr(self, f.name, [] if f.name == "files" else None)


def _none(v):
    return None if v is None or str(v).strip() == "" or str(v).strip().lower() in ("nan", "none") else v


def load_protein_ligand_csv(path: str) -> List[Dict]:
    """Rows of the csv with the cleaning of `load_protein_ligand_df` (datasets/pdbbind.py:1000-1066)."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if _none(r.get("ligand")) is None or _none(r.get("experimental_protein")) is None:
                continue
            c = [_none(r.get(f"pocket_center_{a}")) for a in "xyz"]
            rows.append({"complex_name": r["complex_name"], "experimental_protein": r["experimental_protein"], "ligand": r["ligand"],
                         "pocket_center": [float(v) for v in c] if all(v is not None for v in c) else None,
                         "flexible_sidechains": _none(r.get("flexible_sidechains"))})
    return rows


def _esm_rows(esm_embeddings, name):
    """The ESM embedding stored for a complex (None if there is none): a tensor / array, or a list of per-chain ones."""
    if esm_embeddings is None:
        return None
    if isinstance(esm_embeddings, dict):
        return esm_embeddings.get(name)
    for ext in (".pt", ".npy"):
        p = os.path.join(esm_embeddings, name + ext)
        if os.path.exists(p):
            return torch.load(p, weights_only=True) if ext == ".pt" else np.load(p)
    return None


def read_row_texts(row: Dict, root: str = "") -> Tuple[str, str]:
    """(PDB text, SDF text) of one csv row."""
    lig = row["ligand"]
    if not lig.lower().endswith(".sdf"):
        raise NotImplementedError(f"ligand '{lig}': only SDF files are read without rdkit")
    with open(os.path.join(root, row["experimental_protein"])) as f:
        pdb_text = f.read()
    with open(os.path.join(root, lig)) as f:
        return pdb_text, f.read()


def build_row_graph(row: Dict, esm_embeddings=None, root: str = "", allow_zero_esm: bool = False, texts: Optional[Tuple[str, str]] = None,
                    **graph_kwargs):
    """One csv row -> complex graph (receptor.x = [residue index | 1280 ESM columns]).  The stored embedding may cover the
    whole structure (per chain or concatenated): it is sliced with the kept-residue indices like the reference does
    (inputs.slice_lm_embeddings).  A row without an embedding is an ERROR (-> the row is reported as skipped) unless
    `allow_zero_esm` asks for a zero block, which is out of the model's training distribution and is announced loudly.
    texts: read_row_texts(row, root) where the caller has read the files already."""
    pdb_text, sdf_text = texts or read_row_texts(row, root)
    e = _esm_rows(esm_embeddings, row.get("esm_name", row["complex_name"]))
    if e is None and not allow_zero_esm:
        raise ValueError(f"{row['complex_name']}: no ESM embedding found (pass allow_zero_esm=True to run on a zero block)")
    g = I.build_complex_graph(pdb_text, sdf_text, name=row["complex_name"], pocket_center=row.get("pocket_center"),
                              flexible_sidechains=row.get("flexible_sidechains"), lm_embeddings=e, **graph_kwargs)
    if e is None:
        import warnings
        warnings.warn(f"{row['complex_name']}: no ESM embedding - the receptor gets a ZERO language-model block "
                      f"(out-of-distribution input; allow_zero_esm=True)", RuntimeWarning, stacklevel=2)
        n_res = g["receptor"].x.shape[0]
        g["receptor"].x = torch.cat([g["receptor"].x.float()[:, :1], torch.zeros(n_res, 1280)], 1)
    return g


def run_csv(csv_path: str, model, device, *, confidence_model=None, samples_per_complex: int = 40, inference_steps: int = 20,
            esm_embeddings=None, root: str = "", seed: int = 0, rank: int = 0, world: int = 1, shard: str = "samples",
            dist=None, sampler_cfg: Optional[SamplerConfig] = None, graph_kwargs: Optional[Dict] = None,
            allow_zero_esm: bool = False, evaluate: bool = False, out_dir: Optional[str] = None,
            save_visualisation: bool = False, cluster_rmsd: Optional[float] = None,
            resolve_clashes: Optional[RefineConfig] = None, find_pockets: Optional[PocketConfig] = None,
            pockets_top_k: int = 1, score_poses: Optional[ScoreConfig] = None, rank_by: str = "confidence",
            minimize_poses: Optional[MinimizeConfig] = None, interaction_profile: Optional[ProfileConfig] = None,
            search_poses: Optional[SearchConfig] = None) -> List[ComplexResult]:
    """See the module docstring.  `dist`: an initialised torch.distributed module (world > 1 and shard == "samples").
    Returns one ComplexResult per csv row (on every rank; with shard == "complexes" only this rank's rows are filled).

    A row that fails on ANY rank (unreadable file, unsupported ligand format, missing ESM embedding, a parsing error: every
    Exception, like the reference's per-complex try / except, inference.py:282-287) is skipped on ALL ranks: with sample
    sharding the ranks agree on the outcome (one all_reduce of an ok flag per row) before anyone enters the sampling loop and
    its final all_gather, and once more after sampling and the confidence pass (a sampling-time failure is rank-local: every rank
    holds different poses), so a rank-local failure cannot leave the others waiting in a collective.

    evaluate=True: every processed row also gets `metrics` (evaluation.PoseEvaluator: RMSD, centroid distance, contacts and clashes
    against the input ligand pose - the csv's ligand file is then the known pose - in the ranked order of `ligand_pos`), computed
    after the gather so that every rank holds the full set.  Rigid rows are scored against the row's full PDB (the reference's static
    receptor), flexible rows against the graph's atom nodes at each sample's side-chain positions (+ the side-chain RMSD).  A failure
    of the evaluation skips the row like any other per-row failure.

    out_dir: every processed row also gets the files of reference inference.py:240-280 in `{out_dir}/index{i}___{name}`
    (outputs.write_complex: ranked SDF poses, with flexible side chains the receptors with the moved side chains), listed in
    `files`; save_visualisation=True records the reverse process on the device (SamplerConfig.record_trajectory) and adds
    rank{k}_reverseprocess[_protein].pdb; the trajectories are also returned (`lig_traj`, `atom_traj`, ranked order).  With
    sample sharding the full atom poses and the trajectories are gathered with the ligand poses and rank 0 alone writes (with
    shard="complexes" each rank writes its own rows); a write failure skips the row on every rank.

    cluster_rmsd=X: every processed row also gets `clusters` (evaluation.PoseEvaluator.cluster: the symmetry-corrected RMSD of every
    pair of the gathered poses and their greedy grouping into binding modes at cutoff X, in ranked order: mode 0 holds rank 1), and
    with out_dir the complex directory also gets modes.csv (outputs.write_modes_csv).  Needs no known pose.  A failure skips the row
    like a failure of the evaluation.  None: nothing is computed or written.

    resolve_clashes=RefineConfig(...): after the ranking, the gathered poses also go through refine.PoseRefiner (this package's own
    clash relief in pose space, not the reference's --relax): `refined_pos` and `refine` in ranked order, with evaluate=True also
    `refined_metrics`.  Rigid rows are refined against the row's full PDB, flexible rows against each sample's own atom nodes, as the
    evaluation chooses.  With out_dir the complex directory also gets rank{k}_resolved.sdf per pose and clashes.csv
    (outputs.write_clashes_csv).  Nothing that exists without it changes: ligand_pos, confidences, order, metrics and every other
    file are the same.  A failure skips the row like a failure of the evaluation.  None: nothing is computed or written.

    find_pockets=PocketConfig(...): a row WITHOUT pocket_center_* gets its centre from pockets.find_pockets on the row's protein (this
    package's geometric finder, on `device`): it is docked at the `ca_center` of pocket 1, and with pockets_top_k = K > 1 it is expanded
    into the rows `{name}_pocket{k}`, k = 1 ... min(K, found), each docked, ranked and written like any other row (one ComplexResult
    each, seeds and directory indices counting the expanded rows; the ESM embedding is looked up under the row's own name).  Such a
    result carries `pockets` (all pockets found), and with out_dir its directory gets pockets.csv (outputs.write_pockets_csv: one line
    per pocket found, `docked` = 1 for the pockets this run docked).  A protein on which no pocket survives, or that cannot be read,
    fails the row like any other per-row failure.  A row with an explicit centre keeps it and gets none of this.  None: nothing is
    computed or written, and a row without a centre takes it from the ligand's pose as before.

    score_poses=ScoreConfig(...): the gathered poses also get the Vinardo-form physics score of scoring.PoseScorer (an empirical function
    over ligand-receptor atom pairs; not validated against smina or Vina, no replacement for the confidence model), before the order is
    formed: `scores` in ranked order, with resolve_clashes also `refined_scores`, with out_dir also scores.csv
    (outputs.write_scores_csv).  The receptor is the one the evaluation chooses: the row's full PDB for rigid rows, each sample's own
    atom nodes for flexible rows.  rank_by="score" (implies scoring with the default ScoreConfig) orders the poses by ascending
    `total` instead of by confidence - ties in sample order, NaN last - and everything downstream follows that order: `order`, the
    files, the clustering, the clash relief.  rank_by="confidence" keeps the order described above exactly; without either argument
    nothing is computed or written.  A scoring failure skips the row like a failure of the evaluation.

    minimize_poses=MinimizeConfig(...): the gathered poses, in sample order and right after the scoring, also go through
    minimize.PoseMinimizer: a local descent of every pose in the physics score (score_poses' constants, else the default ScoreConfig)
    along the sampler's degrees of freedom, then rescoring - no receptor motion, no global search, a score that is not validated
    against smina or Vina.  `minimized` (a MinimizeResult) and `minimized_pos` in ranked order; with out_dir also
    rank{k}_minimized.sdf per pose and minimized.csv (outputs.write_minimized_csv).  The receptor is the scoring's: the row's full typed
    PDB for rigid rows, each sample's own atom nodes for flexible rows.  The clash relief is independent of it: both start from the
    sampled poses.  minimize_poses.sidechains=True: a flexible row goes through minimize_flex.FlexPoseMinimizer instead, which moves the
    chi angles of the flexible residues with the ligand (k_sc = minimize_poses.sidechain_restraint); `minimized` is then a
    FlexMinimizeResult, E in minimized.csv the joint E, and with out_dir also rank{k}_minimized_protein.pdb (the receptor with the
    minimised side chains) and minimized_sidechains.csv; rigid rows take the path above.  rank_by="minimized_score" (implies minimisation with the default MinimizeConfig) orders the poses by ascending
    `scores_after.total` through scoring.rank_order, and everything downstream follows that order, as with "score".  Without either
    argument nothing is allocated, launched or written differently.  A failure skips the row like a failure of the evaluation.

    interaction_profile=ProfileConfig(...): the gathered, ranked poses also get the per-residue interaction profile of
    interactions.InteractionProfiler (the pair terms of the physics score - score_poses' constants, else the default ScoreConfig -
    summed per residue, and three bits per residue: contact, hydrophobic, hbond): `interactions` in ranked order, with out_dir also
    interactions.csv, interaction_summary.csv and interaction_similarity.csv (outputs.write_interaction*_csv).  Rigid rows run
    against the row's full typed PDB with the PDB's residue labels, flexible rows against each sample's own atom nodes with the
    graph's.  evaluate=True: `interaction_reference` is the profile of the input ligand pose through the same profiler, and
    interaction_similarity.csv also says how similar every pose's bits are to it and how many of them the pose recovers.  It changes
    nothing else; a failure skips the row like a failure of the evaluation.  None: nothing is computed, allocated, launched or
    written.

    search_poses=SearchConfig(...): the gathered poses, in sample order and right after the minimisation block, also go through
    search.PoseSearcher: every pose seeds `replicas` chains of random move, local descent and Metropolis decision in the physics score
    (score_poses' constants, else the default ScoreConfig), and the best minimum over the chains is the result - never worse in E than
    the minimiser's with the same iteration count, but not Vina's search, without receptor or side-chain motion, and in a score that
    is not validated against smina or Vina (search.py states what it is and is not).  `searched` (a SearchResult) and `searched_pos`
    in ranked order; with out_dir also rank{k}_searched.sdf per pose and searched.csv (outputs.write_searched_csv).  The receptor is
    the scoring's: the row's full typed PDB for rigid rows, each sample's own atom nodes for flexible rows.  It is independent of
    minimize_poses and resolve_clashes: all of them start from the sampled poses.  search_poses.sidechains=True: a flexible row goes
    through search_flex.FlexPoseSearcher instead, which moves the side chains of the flexible residues with the ligand, in the random
    moves and in the descent: `searched` is then a FlexSearchResult, E in searched.csv the joint E, and with out_dir also
    rank{k}_searched_protein.pdb (the receptor with the searched side chains) and searched_sidechains.csv; rigid rows take the path
    above.  rank_by="searched_score" (implies the search with the
    default SearchConfig) orders the poses by ascending `scores_after.total` through scoring.rank_order, and everything downstream
    follows that order.  None: nothing is computed, allocated, launched or written.  A failure skips the row like a failure of the
    evaluation."""
    if rank_by not in ("confidence", "score", "minimized_score", "searched_score"):
        raise ValueError(f"rank_by: 'confidence', 'score', 'minimized_score' or 'searched_score', got {rank_by!r}")
    if rank_by == "searched_score" and search_poses is None:
        search_poses = SearchConfig()
    if rank_by == "score" and score_poses is None:
        score_poses = ScoreConfig()
    if rank_by == "minimized_score" and minimize_poses is None:
        minimize_poses = MinimizeConfig()
    if pockets_top_k < 1:
        raise ValueError("pockets_top_k must be at least 1")
    if sampler_cfg is not None and sampler_cfg.svgd_weight > 0:
        # the samples of a complex interact: a row's sampler would raise inside the per-row try and the row would only be skipped
        if shard == "samples" and world > 1:
            raise ValueError("svgd_weight > 0 needs all samples of a complex on one device: samples cannot be sharded over ranks "
                             "(use shard='complexes')")
        if samples_per_complex < 3:
            raise ValueError("svgd_weight > 0 needs at least 3 samples per complex")
    dev = torch.device(device)
    args = (csv_path, model, dev, confidence_model, samples_per_complex, inference_steps, esm_embeddings, root, seed, rank, world,
            shard, dist, sampler_cfg, graph_kwargs, allow_zero_esm, evaluate, out_dir, save_visualisation, cluster_rmsd, resolve_clashes,
            find_pockets, pockets_top_k, score_poses, rank_by, minimize_poses, interaction_profile, search_poses)
    if dev.type == "cuda":      # kernels are queued on the CURRENT device's stream: make `device` current for the whole run
        with torch.cuda.device(dev):
            return _run_csv(*args)
    return _run_csv(*args)


def _all_ok(dist, ok: bool, device) -> bool:
    """True iff `ok` on every rank."""
    on_gpu = device.type == "cuda" and str(dist.get_backend()).lower() == "nccl"
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device if on_gpu else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    return bool(flag.item())


def _run_csv(csv_path, model, device, confidence_model, samples_per_complex, inference_steps, esm_embeddings, root, seed, rank,
             world, shard, dist, sampler_cfg, graph_kwargs, allow_zero_esm, evaluate=False, out_dir=None,
             save_visualisation=False, cluster_rmsd=None, resolve_clashes=None, find_pockets=None, pockets_top_k=1, score_poses=None,
             rank_by="confidence", minimize_poses=None, interaction_profile=None, search_poses=None) -> List[ComplexResult]:
    rows = load_protein_ligand_csv(csv_path)
    if find_pockets is not None:
        rows = expand_pocket_rows(rows, root, device, find_pockets, pockets_top_k)
    if shard not in ("samples", "complexes"):
        raise ValueError(shard)
    mine = range(len(rows))
    if shard == "complexes" and world > 1:
        mine = np.array_split(np.arange(len(rows)), world)[rank].tolist()      # inference.py:468
    out: List[ComplexResult] = []
    schedule = get_t_schedule(inference_steps)
    for i, row in enumerate(rows):
        res = ComplexResult(name=row["complex_name"], pockets=row.get("pockets"))
        out.append(res)
        if i not in mine:
            continue
        split = shard == "samples" and world > 1
        g = texts = None
        try:
            if row.get("pocket_error") is not None:
                raise ValueError(row["pocket_error"])
            texts = read_row_texts(row, root)      # read once: the graph, the receptor forms of the stages and the writer share them
            g = build_row_graph(row, esm_embeddings, root, allow_zero_esm=allow_zero_esm, texts=texts, **(graph_kwargs or {}))
        except Exception as e:      # noqa: BLE001 - the reference skips a failing complex and goes on (inference.py:282-287)
            res.skipped = f"{type(e).__name__}: {e}"
        if split and not _all_ok(dist, g is not None, device):
            res.skipped = res.skipped or "skipped: the row failed on another rank"
            continue
        if g is None:
            continue
        flex = bool(getattr(model, "flexible_sidechains", False)) and len(g["flexResidues"]) > 0
        cfg = sampler_cfg or SamplerConfig(inference_steps=inference_steps, flexible_sidechains=flex)
        if save_visualisation and not cfg.record_trajectory:
            cfg = dataclasses.replace(cfg, record_trajectory=True)
        moved = flex and cfg.flexible_sidechains       # side chains sampled (else the written receptor is the input's)
        n = samples_per_complex
        sl = slice(rank * n // world, (rank + 1) * n // world) if split else slice(0, n)
        # Sampling can fail on ONE rank only (each rank holds other poses: a truncated ligand<-atom list - DdpError after the run's
        # final synchronisation -, DDP_ELIMIT, out of memory): like the reference (inference.py:282-287) the complex is then
        # skipped - on EVERY rank, agreed before anyone enters the gathers below
        lig = conf = smp = apos = ltraj = atraj = None
        try:
            smp = Sampler(model, g, n, device, cfg, seed=seed + i, sample_slice=sl)
            smp.randomize()
            smp.run(schedule)
            lig = smp.lig_pos
            if ((evaluate or resolve_clashes is not None or score_poses is not None or minimize_poses is not None
                 or interaction_profile is not None or search_poses is not None) and flex) or (out_dir is not None and moved):
                apos = smp.atom_pos.clone()
            if save_visualisation:
                ltraj = smp.lig_traj.clone()
                atraj = smp.atom_traj.clone() if smp.atom_traj is not None else None
            if confidence_model is not None:
                conf, _ = smp.confidence(confidence_model)
        except Exception as e:      # noqa: BLE001
            res.skipped = f"{type(e).__name__}: {e}"
            lig = None
        finally:
            if smp is not None and hasattr(smp, "close"):
                if lig is not None:
                    lig = lig.clone()       # (the poses live in the sampler's buffers)
                smp.close()                 # the captured step's memory goes back to the shared pool before the next complex
        if split and not _all_ok(dist, lig is not None, device):
            res.skipped = res.skipped or "skipped: sampling failed on another rank"
            continue
        if lig is None:
            continue
        if split:
            sizes = [(r + 1) * n // world - r * n // world for r in range(world)]
            lig = _gather_rows(dist, lig, sizes)
            if conf is not None:
                conf = _gather_rows(dist, conf, sizes)
            if apos is not None:
                apos = _gather_rows(dist, apos, sizes)
            if ltraj is not None:
                ltraj = _gather_rows(dist, ltraj, sizes)
            if atraj is not None:
                atraj = _gather_rows(dist, atraj, sizes)
        # From here on every rank holds all poses and runs the same stages in the same order; each enabled stage is one _stage call,
        # and with sample sharding one agreement of the ranks, so no stage may be skipped or reordered on one rank alone.
        tools = _RowTools(row, g, device, flex, score_poses, texts)
        stage = functools.partial(_stage, res, (lambda ok: _all_ok(dist, ok, device)) if split else None)
        scores = minimized = searched = None
        # scoring, minimisation and search run on the gathered poses in sample order: the ranking below may depend on them
        if score_poses is not None:
            scores = stage("scoring", "scoring failed on another rank", lambda: tools.score(lig, apos))
            if scores is None:
                continue
        if minimize_poses is not None:
            minimized = stage("minimisation", "minimisation failed on another rank", lambda: tools.minimize(lig, apos, minimize_poses))
            if minimized is None:
                continue
        if search_poses is not None:
            searched = stage("search", "the search failed on another rank", lambda: tools.search(lig, apos, search_poses))
            if searched is None:
                continue
        if rank_by == "score":
            order = rank_order(scores.total)
        elif rank_by == "searched_score":
            order = rank_order(searched.scores_after.total).to(lig.device)
        elif rank_by == "minimized_score":
            order = rank_order(minimized.scores_after.total).to(lig.device)
        elif conf is not None:      # reference inference.py:212-219: descending confidence (first column of a multi-output head)
            key = conf[:, 0] if conf.dim() == 2 else conf
            order = torch.argsort(key, descending=True)
        else:
            order = torch.arange(lig.shape[0], device=lig.device)
        res.order = order.cpu()
        res.ligand_pos = lig[order].cpu()
        res.confidence = conf[order].cpu() if conf is not None else None
        res.original_center = getattr(g, "original_center", None)
        if scores is not None:
            res.scores = scores.index(order).cpu()
        if minimized is not None:
            res.minimized = minimized.index(order.cpu())
            res.minimized_pos = res.minimized.lig_pos
        if searched is not None:
            res.searched = searched.index(order.cpu())
            res.searched_pos = res.searched.lig_pos
        ranked, apos_ranked = lig[order], None if apos is None else apos[order]
        if evaluate:
            res.metrics = stage("evaluation", "evaluation failed on another rank", lambda: tools.evaluate(ranked, apos_ranked))
            if res.metrics is None:
                continue
        if cluster_rmsd is not None:
            res.clusters = stage("clustering", "clustering failed on another rank", lambda: tools.cluster(ranked, cluster_rmsd))
            if res.clusters is None:
                continue
        if resolve_clashes is not None:
            done = stage("clash relief", "clash relief failed on another rank",
                         lambda: tools.refine(ranked, apos_ranked, resolve_clashes, evaluate))
            if done is None:
                continue
            res.refine, res.refined_metrics, res.refined_scores = done
            res.refined_pos = res.refine.lig_pos
        if interaction_profile is not None:
            done = stage("interaction profile", "the interaction profile failed on another rank",
                         lambda: tools.interactions(ranked, apos_ranked, interaction_profile, evaluate))
            if done is None:
                continue
            res.interactions, res.interaction_reference = done
        if save_visualisation:
            res.lig_traj = ltraj[order].cpu()
            res.atom_traj = atraj[order].cpu() if atraj is not None else None
        if out_dir is not None:      # rank 0 alone writes the gathered poses; the others only agree on its outcome
            files = stage("writing", "writing failed on rank 0",
                          (lambda: tools.write(out_dir, i, res, apos_ranked.cpu() if moved else None, (graph_kwargs or {}).get("remove_hs", True)))
                          if (rank == 0 or not split) else list)
            if files is not None:
                res.files = files
    return out


def _stage(res: ComplexResult, agree, label: str, other: str, fn):
    """One stage of a row of run_csv: what fn() returns (never None), or None where the row ends here.  An exception of fn skips the
    row as `"{label}: ..."`; with sample sharding the ranks then agree (`agree(ok)`: True iff ok on every rank, one collective per
    stage on every rank, whatever happened here) and a failure elsewhere skips the row as `"skipped: {other}"`.  A row that ends
    loses every result it has so far (ComplexResult.clear)."""
    value = None
    try:
        value = fn()
    except Exception as e:      # noqa: BLE001 - the reference skips a failing complex and goes on (inference.py:282-287)
        res.skipped = f"{label}: {type(e).__name__}: {e}"
    if agree is not None and not agree(res.skipped is None):
        res.skipped = res.skipped or f"skipped: {other}"
    if res.skipped is None:
        return value
    res.clear()
    return None


def expand_pocket_rows(rows: List[Dict], root: str, device, config: PocketConfig, top_k: int = 1) -> List[Dict]:
    """run_csv(find_pockets=config): every row without an explicit centre gets `pocket_center` = ca_center of a pocket found on its
    protein, `pockets` (all found) and `pockets_docked` (how many this run docks); with top_k > 1 it becomes the rows
    `{name}_pocket{k}`.  A protein that cannot be read or on which nothing survives leaves ONE row that carries `pocket_error`."""
    out = []
    for row in rows:
        if row.get("pocket_center") is not None:
            out.append(row)
            continue
        try:
            with open(os.path.join(root, row["experimental_protein"])) as f:
                found = _find_pockets(f.read(), device, config)
            if not found:
                raise ValueError(f"{row['complex_name']}: no pocket found on {row['experimental_protein']} (find_pockets: no component of "
                                 f"at least {config.min_points} buried points; give pocket_center_x/y/z, or relax PocketConfig)")
        except Exception as e:      # noqa: BLE001 - reported through the row's own failure path
            out.append(dict(row, pocket_error=f"{type(e).__name__}: {e}" if not isinstance(e, ValueError) else str(e)))
            continue
        k_max = min(top_k, len(found))
        for k in range(k_max):
            name = row["complex_name"] if top_k == 1 else f"{row['complex_name']}_pocket{k + 1}"
            out.append(dict(row, complex_name=name, esm_name=row.get("esm_name", row["complex_name"]),
                            pocket_center=[float(v) for v in found[k].ca_center], pockets=found, pockets_docked=k_max))
    return out


class _RowTools:
    """What the stages of one processed row of run_csv share, each built when a stage first asks for it and at most once: the receptor
    in its three forms and the tools on them.  A rigid row's receptor is the row's full PDB in the graph's frame, a flexible row's the
    graph's atom nodes at each sample's own atom_pos (run_csv keeps an atom_pos for flexible rows only, so it is handed on as it is).
    One method per stage; each returns host tensors.  texts: read_row_texts of the row."""

    def __init__(self, row, g, device, flex, score_poses, texts):
        self.row, self.g, self.device, self.flex, self.score_poses = row, g, device, flex, score_poses
        self.pdb_text, self.sdf_text = texts

    @functools.cached_property
    def full_receptor(self):       # of the evaluation and the clash relief
        return "graph" if self.flex else PoseEvaluator.full_receptor(self.pdb_text, self.g.original_center)

    @functools.cached_property
    def typed_receptor(self):      # of the physics score and everything that descends in it
        return "graph" if self.flex else typed_receptor(self.pdb_text, self.g.original_center)

    @functools.cached_property
    def residues(self):
        return receptor_residues(self.pdb_text)

    @functools.cached_property
    def evaluator(self) -> PoseEvaluator:
        return PoseEvaluator(self.g, self.device, receptor=self.full_receptor)

    @functools.cached_property
    def scorer(self) -> PoseScorer:
        """The one PoseScorer of the row: the minimiser and the searcher run on its tables (score_poses None: the default constants,
        which is what they would build themselves)."""
        return PoseScorer(self.g, self.device, receptor=self.typed_receptor, config=self.score_poses)

    def score(self, lig, apos) -> PoseScores:
        """On the poses' device: the ranking reads it there."""
        return self.scorer.score(lig, apos)

    def minimize(self, lig, apos, config) -> MinimizeResult:
        """A flexible row with config.sidechains: the FlexMinimizeResult of the joint minimisation."""
        if self.flex and config.sidechains:
            return FlexPoseMinimizer(self.g, self.device, score_config=self.score_poses, config=config).minimize(lig, apos).cpu()
        return PoseMinimizer(self.g, self.device, config=config, scorer=self.scorer).minimize(lig, apos).cpu()

    def search(self, lig, apos, config) -> SearchResult:
        """A flexible row with config.sidechains: the FlexSearchResult of the search with the side chains in the state."""
        if self.flex and config.sidechains:
            return FlexPoseSearcher(self.g, self.device, score_config=self.score_poses, config=config).search(lig, apos).cpu()
        return PoseSearcher(self.g, self.device, config=config, scorer=self.scorer).search(lig, apos).cpu()

    def evaluate(self, lig, apos) -> PoseMetrics:
        return self.evaluator.evaluate(lig, apos).cpu()

    def cluster(self, lig, cutoff) -> PoseClusters:
        return PoseEvaluator(self.g, self.device).cluster(lig, None, cutoff).cpu()

    def refine(self, lig, apos, config, evaluate):
        """(RefineResult, PoseMetrics of the refined poses or None, their PoseScores or None)."""
        out = PoseRefiner(self.g, self.device, receptor=self.full_receptor, config=config).refine(lig, apos)
        metrics = self.evaluate(out.lig_pos, apos) if evaluate else None
        scores = self.score(out.lig_pos, apos).cpu() if self.score_poses is not None else None
        return out.cpu(), metrics, scores

    def interactions(self, lig, apos, config, evaluate):
        """(InteractionProfile of the poses, InteractionProfile of the input pose or None)."""
        rec = "graph" if self.flex else (self.typed_receptor, self.residues)
        pf = InteractionProfiler(self.g, self.device, receptor=rec, config=config, score_config=self.score_poses)
        out = pf.profile(lig, apos).cpu()
        ref = pf.profile(torch.as_tensor(self.g["ligand"].pos).float()[None].to(lig.device)).cpu() if evaluate else None
        return out, ref

    def write(self, out_dir, i, res: ComplexResult, apos, remove_hs) -> List[str]:
        """outputs.write_complex of the ranked tensors of `res`."""
        row = self.row
        needs_pdb = apos is not None or res.atom_traj is not None or isinstance(res.minimized, FlexMinimizeResult) or \
            isinstance(res.searched, FlexSearchResult)
        return O.write_complex(O.complex_dir(out_dir, i, row["complex_name"]), self.sdf_text, self.pdb_text if needs_pdb else None, self.g,
                               res.ligand_pos, res.confidence, apos, res.lig_traj, res.atom_traj, remove_hs=remove_hs,
                               clusters=res.clusters, order=res.order, refine=res.refine, pockets=res.pockets,
                               pockets_docked=row.get("pockets_docked", 0), scores=res.scores, refined_scores=res.refined_scores,
                               minimized=res.minimized, interactions=res.interactions,
                               interaction_reference=res.interaction_reference, searched=res.searched)


def _gather_rows(dist, t: torch.Tensor, sizes: Sequence[int]) -> torch.Tensor:
    """all_gather of per-rank row blocks of different lengths (padded to the longest)."""
    pad = max(sizes)
    buf = torch.zeros((pad,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    buf[: t.shape[0]] = t
    parts = [torch.empty_like(buf) for _ in sizes]
    dist.all_gather(parts, buf.contiguous())
    return torch.cat([p[:s] for p, s in zip(parts, sizes)], 0)


# ---------------------------------------------------------------------------------------------- command line
def _guidance_fields(a) -> Dict:
    """The --clash_guidance* and --score_guidance* flags as SamplerConfig fields (clash first, five each, then the two of the
    side-chain part of score guidance)."""
    return dict(clash_guidance_weight=a.clash_guidance, clash_guidance_t_max=a.clash_guidance_t_max,
                clash_guidance_max_tr=a.clash_guidance_max_tr, clash_guidance_max_rot=a.clash_guidance_max_rot,
                clash_guidance_max_tor=a.clash_guidance_max_tor,
                score_guidance_weight=a.score_guidance, score_guidance_t_max=a.score_guidance_t_max,
                score_guidance_max_tr=a.score_guidance_max_tr, score_guidance_max_rot=a.score_guidance_max_rot,
                score_guidance_max_tor=a.score_guidance_max_tor, score_guidance_sidechains=a.score_guidance_sidechains,
                score_guidance_max_sc=a.score_guidance_max_sc)


def _parser():
    """Reference inference.py:49-103: the same flag names and defaults for what this package implements; --esm_embeddings,
    --allow_zero_esm, --device and --seed are this package's."""
    import argparse
    from .sampler import TEMP_PSI, TEMP_SAMPLING, TEMP_SIGMA_DATA
    p = argparse.ArgumentParser(prog="python -m diffdock_pocket_amd.inference",
                                description="Dock SDF ligands into PDB pockets and write ranked poses (one process).")
    p.add_argument("--complex_name", type=str, default="unnamed_complex")
    p.add_argument("--protein_ligand_csv", type=str, default=None)
    p.add_argument("--protein_path", "--experimental_protein", type=str, default=None)
    p.add_argument("--ligand", type=str, default="COc(cc1)ccc1C#N", help="an SDF file (SMILES and other formats need rdkit: not read)")
    p.add_argument("--flexible_sidechains", type=str, default=None)
    p.add_argument("--out_dir", type=str, default="results/user_inference")
    p.add_argument("--save_visualisation", action="store_true", default=False)
    p.add_argument("--samples_per_complex", type=int, default=10)
    p.add_argument("--rigid", action="store_true", default=False)
    for a in "xyz":
        p.add_argument(f"--pocket_center_{a}", type=float, default=None)
    p.add_argument("--model_dir", type=str, default=None, help="score model: model_parameters.yml + checkpoint (required: no download)")
    p.add_argument("--ckpt", type=str, default="best_ema_inference_epoch_model.pt")
    p.add_argument("--filtering_model_dir", type=str, default=None)
    p.add_argument("--filtering_ckpt", type=str, default="best_model.pt")
    p.add_argument("--no_random", action="store_true", default=False)
    p.add_argument("--no_final_step_noise", action="store_true", default=False)
    p.add_argument("--ode", action="store_true", default=False)
    p.add_argument("--inference_steps", type=int, default=30)
    for k, name in enumerate(("tr", "rot", "tor", "sc_tor")):
        p.add_argument(f"--temp_sampling_{name}", type=float, default=TEMP_SAMPLING[k])
        p.add_argument(f"--temp_psi_{name}", type=float, default=TEMP_PSI[k])
    p.add_argument("--temp_sigma_data", type=float, default=TEMP_SIGMA_DATA)
    p.add_argument("--svgd_weight", type=float, default=0.0, help="> 0: add the SVGD particle-interaction term (rigid receptor, >= 3 samples)")
    p.add_argument("--svgd_repulsive_weight", type=float, default=1.0)
    p.add_argument("--svgd_only", action="store_true", default=False, help="the SVGD term replaces the SDE / ODE update")
    p.add_argument("--svgd_rot_rel_weight", type=float, default=1.0)
    p.add_argument("--svgd_tor_rel_weight", type=float, default=1.0)
    p.add_argument("--clash_guidance", type=float, default=0.0, metavar="W",
                   help="> 0: nudge every denoising step down the gradient of the steric-clash energy with this per-step weight "
                        "(guidance.py; untuned, not validated on real checkpoints; default: off)")
    p.add_argument("--clash_guidance_t_max", type=float, default=1.0, help="guide only the steps with diffusion time t <= this")
    p.add_argument("--clash_guidance_max_tr", type=float, default=1.0, help="cap of the guidance translation per step (Angstrom)")
    p.add_argument("--clash_guidance_max_rot", type=float, default=0.5, help="cap of the guidance rotation per step (rad)")
    p.add_argument("--clash_guidance_max_tor", type=float, default=0.5, help="cap of the guidance torsion step per bond (rad)")
    p.add_argument("--score_guidance", type=float, default=0.0, metavar="W",
                   help="> 0: nudge every denoising step down the gradient of the Vinardo-form physics score (inter + intra, the "
                        "graph's pocket atoms) with this per-step weight (score_guidance.py; untuned, not validated on real "
                        "checkpoints; default: off)")
    p.add_argument("--score_guidance_t_max", type=float, default=1.0, help="guide only the steps with diffusion time t <= this")
    p.add_argument("--score_guidance_max_tr", type=float, default=1.0, help="cap of the score-guidance translation per step (Angstrom)")
    p.add_argument("--score_guidance_max_rot", type=float, default=0.5, help="cap of the score-guidance rotation per step (rad)")
    p.add_argument("--score_guidance_max_tor", type=float, default=0.5, help="cap of the score-guidance torsion step per bond (rad)")
    p.add_argument("--score_guidance_sidechains", action="store_true",
                   help="with --score_guidance in a flexible run: guide the side-chain updates too, down the joint energy inter + intra + "
                        "sc of the joint minimiser with respect to the chi angles (score_guidance.py; untuned, no backbone motion, no "
                        "rotamer library); a no-op on a rigid run")
    p.add_argument("--score_guidance_max_sc", type=float, default=0.5, help="cap of the score-guidance side-chain step per bond (rad)")
    p.add_argument("--cluster_rmsd", type=float, default=None,
                   help="group the ranked poses into binding modes at this symmetry-corrected RMSD cutoff and write modes.csv (default: off)")
    p.add_argument("--resolve_clashes", action="store_true", default=False,
                   help="push the ranked poses out of steric clashes in pose space (this package's own refinement, no force field) and "
                        "write rank{k}_resolved.sdf and clashes.csv beside the unchanged poses (default: off)")
    p.add_argument("--resolve_clashes_iterations", type=int, default=RefineConfig.iterations)
    p.add_argument("--resolve_clashes_restraint", type=float, default=RefineConfig.restraint,
                   help="weight of the restraint to the sampled pose")
    p.add_argument("--score_poses", action="store_true", default=False,
                   help="score every pose with this package's Vinardo-form empirical function (not validated against smina or Vina) and "
                        "write scores.csv (default: off)")
    p.add_argument("--rank_by", type=str, choices=("confidence", "score", "minimized_score", "searched_score"), default="confidence",
                   help="order of the written poses: the confidence model's (without one: sample order), ascending physics score "
                        "(implies --score_poses), ascending physics score after the minimisation (implies --minimize_poses), or after the search (implies "
                        "--search_poses)")
    p.add_argument("--minimize_poses", action="store_true", default=False,
                   help="minimise every pose locally in the physics score along translation, rotation and torsions (no receptor motion, "
                        "no global search) and write rank{k}_minimized.sdf and minimized.csv beside the unchanged poses (default: off)")
    p.add_argument("--minimize_iterations", type=int, default=MinimizeConfig.iterations)
    p.add_argument("--minimize_restraint", type=float, default=MinimizeConfig.restraint,
                   help="weight of the restraint to the sampled pose")
    p.add_argument("--minimize_sidechains", action="store_true", default=False,
                   help="implies --minimize_poses; flexible rows: the chi angles of the flexible residues are minimised together with "
                        "the ligand (this package's own local descent, not the reference's --relax) and rank{k}_minimized_protein.pdb and "
                        "minimized_sidechains.csv are written too; rigid rows are minimised as without the flag (default: off)")
    p.add_argument("--minimize_sidechain_restraint", type=float, default=MinimizeConfig.sidechain_restraint,
                   help="with --minimize_sidechains: weight of the restraint of the moving side-chain atoms to their sampled positions")
    p.add_argument("--search_poses", action="store_true", default=False,
                   help="search around every pose in the physics score: replicas of random move, local descent and Metropolis decision "
                        "(not Vina's search, no receptor motion, a score not validated against smina or Vina); writes rank{k}_searched.sdf "
                        "and searched.csv beside the unchanged poses (default: off)")
    p.add_argument("--search_replicas", type=int, default=SearchConfig.replicas, help="with --search_poses: independent chains per pose")
    p.add_argument("--search_cycles", type=int, default=SearchConfig.cycles, help="with --search_poses: cycles per chain")
    p.add_argument("--search_iterations", type=int, default=SearchConfig.iterations,
                   help="with --search_poses: line-search iterations of the local descent of one cycle")
    p.add_argument("--search_temperature", type=float, default=SearchConfig.temperature,
                   help="with --search_poses: temperature of the Metropolis rule, in units of the score")
    p.add_argument("--search_seed", type=int, default=SearchConfig.seed, help="with --search_poses: seed of the random moves")
    p.add_argument("--search_sidechains", action="store_true", default=False,
                   help="implies --search_poses; rows with flexible residues search the chi angles of those residues together with the "
                        "ligand (search_flex.py: Gaussian chi moves around the current rotamer, the joint descent of --minimize_sidechains; "
                        "no backbone motion, no rotamer library): rank{k}_searched_protein.pdb and searched_sidechains.csv are written too; "
                        "rigid rows are searched as without the flag; independent of --minimize_sidechains (default: off)")
    p.add_argument("--search_sigma_chi", type=float, default=SearchConfig.sigma_chi,
                   help="with --search_sidechains: standard deviation of the random side-chain steps, rad per bond")
    p.add_argument("--search_sidechain_restraint", type=float, default=SearchConfig.sidechain_restraint,
                   help="with --search_sidechains: weight of the restraint of the moving side-chain atoms to their sampled positions")
    p.add_argument("--interaction_profile", action="store_true", default=False,
                   help="say which residues every pose touches and how: the pair terms of the physics score summed per residue, with "
                        "contact / hydrophobic / hbond bits (not validated against PLIP or ProLIF); writes interactions.csv, "
                        "interaction_summary.csv and interaction_similarity.csv (default: off)")
    p.add_argument("--interaction_contact_distance", type=float, default=ProfileConfig.contact_distance,
                   help="with --interaction_profile: a residue is in contact when its closest atom pair is nearer than this (angstrom)")
    p.add_argument("--find_pockets", action="store_true", default=False,
                   help="complexes without --pocket_center_* / pocket_center columns: find the pocket on the protein's geometry (this "
                        "package's grid buriedness finder, no learned predictor) and dock there; writes pockets.csv (default: off)")
    p.add_argument("--pockets_top_k", type=int, default=1, help="with --find_pockets: dock into the best K pockets, as complexes {name}_pocket{k}")
    p.add_argument("--pocket_spacing", type=float, default=PocketConfig.spacing, help="grid spacing of the pocket finder, angstrom")
    p.add_argument("--pocket_min_lines", type=int, default=PocketConfig.min_lines, help="lines (of 7) that must be blocked on both sides")
    p.add_argument("--pocket_probe", type=float, default=PocketConfig.probe, help="probe radius added to the van der Waals radii")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--esm_embeddings", type=str, default=None,
                   help="directory of <complex_name>.pt / .npy ESM rows, or one .pt file holding {complex_name: rows}")
    p.add_argument("--allow_zero_esm", action="store_true", default=False,
                   help="run complexes without an ESM embedding on a zero block (out of the model's training distribution)")
    p.add_argument("--device", type=str, default=None, help="default: cuda:0 when a GPU is visible, else cpu")
    return p


def pocket_config_from_args(a) -> Optional[PocketConfig]:
    """The PocketConfig the command line asks for (None without --find_pockets)."""
    if not a.find_pockets:
        return None
    return PocketConfig(spacing=a.pocket_spacing, min_lines=a.pocket_min_lines, probe=a.pocket_probe)


def _load_model(model_dir, ckpt, device, confidence_mode=False):
    """(model, yml namespace): factory.get_model on model_parameters.yml, the checkpoint loaded strictly (inference.py:433-450)."""
    import argparse
    import functools
    import yaml
    from .diffusion import SigmaRanges, t_to_sigma
    from .factory import get_model
    with open(os.path.join(model_dir, "model_parameters.yml")) as f:
        args = argparse.Namespace(**yaml.full_load(f))
    sigma = SigmaRanges(**{k: float(getattr(args, k)) for k in SigmaRanges.__dataclass_fields__ if hasattr(args, k)})
    model = get_model(args, device, functools.partial(t_to_sigma, args=sigma), no_parallel=True, confidence_mode=confidence_mode)
    model.load_state_dict(torch.load(os.path.join(model_dir, ckpt), map_location="cpu", weights_only=True), strict=True)
    return model.to(device).eval(), args, sigma


def _search_config(a) -> Optional[SearchConfig]:
    """The SearchConfig of the parsed flags, or None: --search_sidechains and --rank_by searched_score imply --search_poses."""
    if not (a.search_poses or a.search_sidechains or a.rank_by == "searched_score"):
        return None
    return SearchConfig(replicas=a.search_replicas, cycles=a.search_cycles, iterations=a.search_iterations, temperature=a.search_temperature,
                        seed=a.search_seed, sidechains=a.search_sidechains, sigma_chi=a.search_sigma_chi,
                        sidechain_restraint=a.search_sidechain_restraint)


def main(argv: Optional[Sequence[str]] = None) -> int:
    """The command line: `python -m diffdock_pocket_amd.inference --protein_path P --ligand L.sdf --model_dir M ...` or
    `--protein_ligand_csv C`.  Writes `{out_dir}/index{i}___{name}` per complex (run_csv(out_dir=...)); returns 0 when every
    complex was processed, 1 otherwise."""
    import tempfile
    ap = _parser()
    a = ap.parse_args(argv)
    if a.protein_ligand_csv is not None and a.protein_path is not None:
        ap.error("give either --protein_ligand_csv or --protein_path, not both")
    if a.protein_ligand_csv is None and a.protein_path is None:
        ap.error("either --protein_ligand_csv or --protein_path has to be given")
    if a.model_dir is None or not os.path.isfile(os.path.join(a.model_dir, "model_parameters.yml")):
        ap.error(f"--model_dir {a.model_dir!r}: a directory with model_parameters.yml and the checkpoint is required "
                 f"(models are not downloaded)")
    if a.filtering_model_dir is not None and not os.path.isfile(os.path.join(a.filtering_model_dir, "model_parameters.yml")):
        ap.error(f"--filtering_model_dir {a.filtering_model_dir!r} holds no model_parameters.yml")
    if a.resolve_clashes_iterations < 0 or a.resolve_clashes_restraint < 0:
        ap.error("--resolve_clashes_iterations and --resolve_clashes_restraint must not be negative")
    if a.minimize_iterations < 0 or not a.minimize_restraint >= 0:
        ap.error("--minimize_iterations and --minimize_restraint must not be negative")
    if not a.minimize_sidechain_restraint >= 0:
        ap.error("--minimize_sidechain_restraint must not be negative")
    if not a.search_sigma_chi >= 0:
        ap.error("--search_sigma_chi must not be negative")
    if not a.search_sidechain_restraint >= 0:
        ap.error("--search_sidechain_restraint must not be negative")
    if a.search_replicas < 1 or a.search_cycles < 0 or a.search_iterations < 0 or not (0 < a.search_temperature < float("inf")):
        ap.error("--search_replicas must be at least 1, --search_cycles and --search_iterations not negative, --search_temperature "
                 "positive and finite")
    if a.pockets_top_k < 1 or not a.pocket_spacing > 0 or not 0 <= a.pocket_min_lines <= 7 or a.pocket_probe < 0:
        ap.error("--pockets_top_k must be at least 1, --pocket_spacing positive, --pocket_min_lines in 0..7, --pocket_probe not negative")
    if not (a.interaction_contact_distance > 0 and np.isfinite(a.interaction_contact_distance)):
        ap.error("--interaction_contact_distance must be positive and finite")
    if a.samples_per_complex < 1 or a.inference_steps < 1:
        ap.error("--samples_per_complex and --inference_steps must be positive")
    device = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model, margs, sigma = _load_model(a.model_dir, a.ckpt, device)
    conf_model = _load_model(a.filtering_model_dir, a.filtering_ckpt, device, confidence_mode=True)[0] \
        if a.filtering_model_dir is not None else None
    flexible = bool(getattr(margs, "flexible_sidechains", False)) and not a.rigid
    graph_kwargs = {k: getattr(margs, k) for k in ("receptor_radius", "c_alpha_max_neighbors", "remove_hs", "pocket_reduction",
                                                   "pocket_buffer", "pocket_cutoff") if hasattr(margs, k)}
    if flexible and getattr(margs, "flexdist", None) is not None:
        graph_kwargs["flexdist"] = float(margs.flexdist)
    try:
        from .guidance import check_config
        fields = list(_guidance_fields(a).values())
        check_config(*fields[:5])
        check_config(*fields[5:10], prefix="score_guidance")
        if not a.score_guidance_max_sc >= 0.0:
            raise ValueError(f"score_guidance_max_sc must not be negative or NaN, got {a.score_guidance_max_sc!r}")
    except ValueError as e:
        msg = str(e)
        for kind in ("clash", "score"):
            msg = msg.replace(f"{kind}_guidance_weight", f"--{kind}_guidance").replace(f"{kind}_guidance_", f"--{kind}_guidance_")
        ap.error(msg)
    cfg = SamplerConfig(inference_steps=a.inference_steps, sigma=sigma,
                        temp_sampling=[a.temp_sampling_tr, a.temp_sampling_rot, a.temp_sampling_tor, a.temp_sampling_sc_tor],
                        temp_psi=[a.temp_psi_tr, a.temp_psi_rot, a.temp_psi_tor, a.temp_psi_sc_tor], temp_sigma_data=a.temp_sigma_data,
                        no_final_step_noise=a.no_final_step_noise, no_random=a.no_random, ode=a.ode, flexible_sidechains=flexible,
                        no_torsion=bool(getattr(margs, "no_torsion", False)), record_trajectory=a.save_visualisation,
                        svgd_weight=a.svgd_weight, svgd_repulsive_weight=a.svgd_repulsive_weight, svgd_only=a.svgd_only,
                        svgd_rot_rel_weight=a.svgd_rot_rel_weight, svgd_tor_rel_weight=a.svgd_tor_rel_weight, **_guidance_fields(a))
    if a.svgd_weight > 0 and (flexible or a.samples_per_complex < 3):
        ap.error("--svgd_weight > 0 needs a rigid receptor (--rigid or a model without flexible side chains) and "
                 "--samples_per_complex >= 3")
    esm = a.esm_embeddings
    if esm is not None and os.path.isfile(esm):
        esm = torch.load(esm, map_location="cpu", weights_only=False)
    os.makedirs(a.out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        csv_path = a.protein_ligand_csv
        if csv_path is None:      # one complex from the flags: a one-row csv (inference.py:351-361)
            csv_path = os.path.join(tmp, "input.csv")
            centre = [a.pocket_center_x, a.pocket_center_y, a.pocket_center_z]
            with open(csv_path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["complex_name", "experimental_protein", "ligand", "pocket_center_x", "pocket_center_y", "pocket_center_z",
                            "flexible_sidechains"])
                w.writerow([a.complex_name, a.protein_path, a.ligand] + ["" if c is None else repr(c) for c in centre]
                           + [a.flexible_sidechains or ""])
        if a.rigid:       # no flexible residues in the graphs (the csv's flexible_sidechains column is ignored)
            rows = load_protein_ligand_csv(csv_path)
            rigid_csv = os.path.join(tmp, "rigid.csv")
            with open(rigid_csv, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["complex_name", "experimental_protein", "ligand", "pocket_center_x", "pocket_center_y", "pocket_center_z"])
                for r in rows:
                    w.writerow([r["complex_name"], r["experimental_protein"], r["ligand"]]
                               + (["", "", ""] if r["pocket_center"] is None else [repr(c) for c in r["pocket_center"]]))
            csv_path = rigid_csv
        res = run_csv(csv_path, model, device, confidence_model=conf_model, samples_per_complex=a.samples_per_complex,
                      inference_steps=a.inference_steps, esm_embeddings=esm, seed=a.seed, sampler_cfg=cfg, graph_kwargs=graph_kwargs,
                      allow_zero_esm=a.allow_zero_esm, out_dir=a.out_dir, save_visualisation=a.save_visualisation,
                      cluster_rmsd=a.cluster_rmsd,
                      resolve_clashes=RefineConfig(iterations=a.resolve_clashes_iterations, restraint=a.resolve_clashes_restraint)
                      if a.resolve_clashes else None,
                      find_pockets=pocket_config_from_args(a), pockets_top_k=a.pockets_top_k,
                      score_poses=ScoreConfig() if (a.score_poses or a.rank_by == "score") else None, rank_by=a.rank_by,
                      minimize_poses=MinimizeConfig(iterations=a.minimize_iterations, restraint=a.minimize_restraint,
                                                    sidechains=a.minimize_sidechains, sidechain_restraint=a.minimize_sidechain_restraint)
                      if (a.minimize_poses or a.minimize_sidechains or a.rank_by == "minimized_score") else None,
                      interaction_profile=ProfileConfig(contact_distance=a.interaction_contact_distance) if a.interaction_profile else None,
                      search_poses=_search_config(a))
    failed = [r for r in res if r.skipped is not None]
    for r in res:
        print(f"{r.name}: " + (f"skipped ({r.skipped})" if r.skipped else f"{len(r.files)} files"), flush=True)
    print(f"{len(res) - len(failed)} of {len(res)} complexes written to {a.out_dir}", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
