"""The stage chain of run_csv (diffdock_pocket_amd/inference.py: _RowTools, _stage, ComplexResult.clear) and the checks and tables the
pose tools share (pose_args.py, scoring.typed_tables, PoseMinimizer / PoseSearcher(scorer=...)), without a device: a run with every
stage on gives each stage what a run with that stage alone gives; a rigid row opens and parses its receptor once per form; a failure
of any stage empties the row under that stage's label and the next row goes on; the argument checks say what they said before they
were shared; a shared scorer changes no bit."""
import builtins
import dataclasses
import os

import pytest
import torch

from diffdock_pocket_amd import evaluation as EV
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import interactions as IA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import pose_args as PA
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd import search as SE
from test_inference_csv import Stub, StubConfidence
from test_scoring_cpu import CSV, GOLDEN, fixture_3dpf, perturbed_poses

HEAD = "complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
MIN = M.MinimizeConfig(iterations=3)
SEARCH = SE.SearchConfig(replicas=2, cycles=2, iterations=3)
# run_csv argument -> (its value here, the ComplexResult field it fills)
STAGES = {"score_poses": (SC.ScoreConfig(), "scores"), "minimize_poses": (MIN, "minimized"), "search_poses": (SEARCH, "searched"),
          "interaction_profile": (IA.ProfileConfig(), "interactions"), "resolve_clashes": (R.RefineConfig(iterations=3), "refine"),
          "evaluate": (True, "metrics"), "cluster_rmsd": (2.0, "clusters")}


def _run(csv_path, **kw):
    return INF.run_csv(str(csv_path), Stub(), torch.device("cpu"), confidence_model=StubConfidence(), samples_per_complex=3,
                       inference_steps=2, root=GOLDEN, seed=2, allow_zero_esm=True, **kw)


def same(a, b, where=""):
    """Every tensor of two results torch.equal (NaN equal to NaN), every other value equal."""
    assert type(a) is type(b), where
    if dataclasses.is_dataclass(a):
        for f in dataclasses.fields(a):
            same(getattr(a, f.name), getattr(b, f.name), f"{where}.{f.name}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape, where
        if a.is_floating_point():
            assert torch.equal(torch.isnan(a), torch.isnan(b)), where
            a, b = torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)
        assert torch.equal(a, b), where
    else:
        assert a == b, where


# ---------------------------------------------------------------------------------------------- 1. combined run = single-stage runs
def test_every_stage_of_a_combined_run_equals_its_solo_run(tmp_path):
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)      # a flexible and a rigid row
    combined = _run(p, **{k: v for k, (v, _) in STAGES.items()})
    assert [r.skipped for r in combined] == [None, None]
    for arg, (value, field) in STAGES.items():
        solo = _run(p, **{arg: value})
        for c, s in zip(combined, solo):
            assert s.skipped is None and getattr(s, field) is not None, (arg, s.skipped)
            assert torch.equal(c.order, s.order) and torch.equal(c.ligand_pos, s.ligand_pos), arg      # both ranked by confidence
            same(getattr(c, field), getattr(s, field), f"{c.name}.{field}")
            for _, other in STAGES.values():      # a solo run fills its own field alone
                assert other == field or getattr(s, other) is None, (arg, other)


# ---------------------------------------------------------------------------------------------- 2. the receptor is read once
def test_a_rigid_row_opens_its_receptor_once_and_builds_each_form_once(tmp_path, monkeypatch):
    p = tmp_path / "one.csv"
    p.write_text(HEAD + "3dpf_rigid,3dpf_protein.pdb,3dpf_ligand.sdf\n")
    pdb = os.path.join(GOLDEN, "3dpf_protein.pdb")
    calls = {"open": 0, "parse_pdb": 0, "full_receptor": 0, "typed_receptor": 0, "receptor_residues": 0}

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    real_open = builtins.open

    def counting_open(file, *a, **k):
        if isinstance(file, (str, os.PathLike)) and os.path.abspath(os.fspath(file)) == pdb:
            calls["open"] += 1
        return real_open(file, *a, **k)

    monkeypatch.setattr(builtins, "open", counting_open)
    counting_parse = counted("parse_pdb", I.parse_pdb)
    for mod in (I, SC, IA):      # evaluation.py looks parse_pdb up in inputs at call time
        monkeypatch.setattr(mod, "parse_pdb", counting_parse)
    monkeypatch.setattr(EV.PoseEvaluator, "full_receptor", staticmethod(counted("full_receptor", EV.PoseEvaluator.full_receptor)))
    monkeypatch.setattr(INF, "typed_receptor", counted("typed_receptor", INF.typed_receptor))
    monkeypatch.setattr(INF, "receptor_residues", counted("receptor_residues", INF.receptor_residues))
    res = _run(p, out_dir=str(tmp_path / "out"), save_visualisation=True, **{k: v for k, (v, _) in STAGES.items()})
    assert res[0].skipped is None and res[0].files
    assert calls["open"] == 1, calls
    assert calls["full_receptor"] == 1 and calls["typed_receptor"] == 1 and calls["receptor_residues"] == 1, calls
    assert calls["parse_pdb"] == 4, calls      # the graph and the three forms


# ---------------------------------------------------------------------------------------------- 3. one failure per stage
KEPT = ("name", "skipped", "pockets", "original_center")
_CACHE = {}


@pytest.mark.parametrize("label,method,arg", [
    ("scoring", "score", None), ("minimisation", "minimize", "minimize_poses"), ("search", "search", "search_poses"),
    ("evaluation", "evaluate", None), ("clustering", "cluster", "cluster_rmsd"), ("clash relief", "refine", "resolve_clashes"),
    ("interaction profile", "interactions", "interaction_profile"), ("writing", "write", None)])
def test_a_failing_stage_empties_its_row_and_the_next_row_goes_on(tmp_path, monkeypatch, label, method, arg):
    """Scoring and evaluation are on in every case, so a later stage has earlier results to clear: `scores` from before the ranking,
    `metrics` from after it (a write failure used to leave `metrics` behind)."""
    p = tmp_path / "two.csv"
    p.write_text(HEAD + "first,3dpf_protein.pdb,3dpf_ligand.sdf\nsecond,3dpf_protein.pdb,3dpf_ligand.sdf\n")
    real = getattr(INF._RowTools, method)

    def failing(self, *a, **k):
        if self.row["complex_name"] == "first":
            raise RuntimeError("made to fail")
        return real(self, *a, **k)

    monkeypatch.setattr(INF._RowTools, method, failing)
    kw = dict(score_poses=SC.ScoreConfig(), evaluate=True, out_dir=str(tmp_path / "out"))
    if arg is not None:
        kw[arg] = STAGES[arg][0]
    first, second = _run(p, **kw)
    assert first.skipped == f"{label}: RuntimeError: made to fail"
    for f in dataclasses.fields(first):
        if f.name not in KEPT:
            assert getattr(first, f.name) == ([] if f.name == "files" else None), f.name
    assert first.name == "first" and first.pockets is None
    assert (first.original_center is not None) == (label not in ("scoring", "minimisation", "search"))      # set with the ranking
    assert second.skipped is None and second.ligand_pos.shape[0] == 3 and second.scores is not None and second.metrics is not None
    assert second.files and (arg is None or getattr(second, STAGES[arg][1]) is not None)
    assert not os.path.exists(os.path.join(str(tmp_path / "out"), "index0___first"))


def test_a_stage_enters_the_agreement_once_whatever_happened_and_takes_the_other_ranks_failure():
    def boom():
        raise KeyError("k")

    for fn, all_ok, value, flag, skipped in (
            (lambda: 7, True, 7, True, None), (lambda: 7, False, None, True, "skipped: scoring failed on another rank"),
            (boom, False, None, False, "scoring: KeyError: 'k'")):
        res, entered = INF.ComplexResult(name="x", confidence=torch.zeros(1)), []
        got = INF._stage(res, lambda ok: entered.append(ok) or all_ok, "scoring", "scoring failed on another rank", fn)
        assert got == value and entered == [flag] and res.skipped == skipped
        assert (res.confidence is None) == (skipped is not None)
    res = INF.ComplexResult(name="x")      # one process: no agreement to enter
    assert INF._stage(res, None, "scoring", "unused", lambda: 7) == 7 and INF._stage(res, None, "scoring", "unused", boom) is None
    assert res.skipped == "scoring: KeyError: 'k'"


def test_clear_keeps_what_names_the_row_and_resets_the_rest():
    full = INF.ComplexResult(**{f.name: f.name for f in dataclasses.fields(INF.ComplexResult)})
    full.clear()
    for f in dataclasses.fields(full):
        assert getattr(full, f.name) == (f.name if f.name in KEPT else [] if f.name == "files" else None), f.name


# ---------------------------------------------------------------------------------------------- 4. the shared argument checks
def _tools():
    g, _, rec = fixture_3dpf()
    return {"scorer": SC.PoseScorer(g, receptor=rec).score, "refiner": R.PoseRefiner(g).refine,
            "profiler": IA.InteractionProfiler(g).profile, "evaluator": EV.PoseEvaluator(g).evaluate}


@pytest.mark.parametrize("who", ["scorer", "refiner", "profiler", "evaluator"])
@pytest.mark.parametrize("fault", ["rank", "n", "n_a", "samples"])
def test_the_pose_tools_refuse_wrong_shapes_in_the_words_they_always_used(who, fault):
    g, _, _ = fixture_3dpf()
    n, n_a = g["ligand"].pos.shape[0], g["atom"].pos.shape[0]
    lig, atom = torch.zeros(2, n, 3), torch.zeros(2, n_a, 3)
    if fault == "rank":
        lig, want = lig[0], f"lig_pos: expected [S, {n}, 3], got ({n}, 3)"
    elif fault == "n":
        lig, want = torch.zeros(2, n + 1, 3), f"lig_pos: expected [S, {n}, 3], got (2, {n + 1}, 3)"
    elif fault == "n_a":
        atom, want = torch.zeros(2, n_a + 1, 3), f"atom_pos: expected [S, {n_a}, 3], got (2, {n_a + 1}, 3)"
    else:
        atom, want = torch.zeros(3, n_a, 3), f"atom_pos: expected [S, {n_a}, 3], got (3, {n_a}, 3)"
    if "tools" not in _CACHE:
        _CACHE["tools"] = _tools()
    with pytest.raises(ValueError) as e:
        _CACHE["tools"][who](lig, atom)
    assert str(e.value) == want


def test_check_poses_and_check_anchor_directly():
    dev = torch.device("cpu")
    lig, atom = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    PA.check_poses(5, 7, dev, lig, atom, "scorer")
    PA.check_poses(5, 7, dev, lig, None, "scorer")
    PA.check_poses(5, 7, None, lig, atom, "evaluator")
    with pytest.raises(ValueError) as e:
        PA.check_poses(5, 7, dev, lig, atom.to("meta"), "scorer")
    assert str(e.value) == "lig_pos and atom_pos on different devices"
    PA.check_poses(5, 7, None, lig, atom.to("meta"), "evaluator")      # device None: the shapes alone, as PoseEvaluator.evaluate tests them
    PA.check_anchor(lig, lig.clone())
    for bad in (torch.zeros(3, 5, 3), torch.zeros(2, 5, 3, device="meta")):
        with pytest.raises(ValueError) as e:
            PA.check_anchor(lig, bad)
        assert str(e.value) == "anchor: the shape and device of lig_pos"


@pytest.mark.parametrize("entry", ["refiner.energy", "minimizer.energy", "minimizer.advance"])
def test_a_mismatched_anchor_is_refused_in_the_words_always_used(entry):
    g, _, rec = fixture_3dpf()
    x = perturbed_poses()[:2]
    bad = x[:1]
    with pytest.raises(ValueError) as e:
        if entry == "refiner.energy":
            R.PoseRefiner(g).energy(x, bad)
        elif entry == "minimizer.energy":
            M.PoseMinimizer(g, receptor=rec).energy(x, bad)
        else:
            M.PoseMinimizer(g, receptor=rec).advance(x, bad, torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 1)
    assert str(e.value) == "anchor: the shape and device of lig_pos"


def test_typed_tables_keeps_the_asymmetry_between_scorer_and_profiler():
    g, _, rec = fixture_3dpf()
    n_a = g["atom"].pos.shape[0]
    typed = int((SC.type_receptor_graph(g)[0] >= 0).sum())
    assert SC.PoseScorer(g)._cpu["rec"].shape[0] == n_a             # a per-sample atom_pos has all n_a rows
    assert IA.InteractionProfiler(g)._cpu["rec"].shape[0] == typed  # indexed with `keep`
    kept = int((rec.radii >= 0).sum())
    assert SC.PoseScorer(g, receptor=rec)._cpu["rec"].shape[0] == kept
    assert IA.InteractionProfiler(g, receptor=(rec, IA.receptor_residues(fixture_3dpf()[1])))._cpu["rec"].shape[0] == kept
    with pytest.raises(ValueError) as e:
        SC.PoseScorer(g, receptor="pdb")
    assert str(e.value) == "receptor: 'graph' or a TypedReceptor, got 'pdb'"
    with pytest.raises(ValueError) as e:
        SC.PoseScorer(g, receptor=(rec, None))
    assert str(e.value) == "receptor: 'graph' or a TypedReceptor, got tuple"
    with pytest.raises(ValueError) as e:
        IA.InteractionProfiler(g, receptor="pdb")
    assert str(e.value) == "receptor: 'graph' or (TypedReceptor, ResidueTable), got 'pdb'"
    with pytest.raises(ValueError) as e:
        IA.InteractionProfiler(g, receptor=rec)
    assert str(e.value) == "receptor: 'graph' or (TypedReceptor, ResidueTable), got TypedReceptor"


# ---------------------------------------------------------------------------------------------- 5. a shared scorer
def test_a_shared_scorer_gives_the_bits_of_separately_built_tools():
    g, _, rec = fixture_3dpf()
    x = perturbed_poses()[:3]
    cfg = SC.ScoreConfig(w_hbond=-0.5)      # not the default: the shared scorer's constants have to arrive
    s = SC.PoseScorer(g, receptor=rec, config=cfg)
    same(M.PoseMinimizer(g, config=MIN, scorer=s).minimize(x), M.PoseMinimizer(g, receptor=rec, score_config=cfg, config=MIN).minimize(x))
    same(SE.PoseSearcher(g, config=SEARCH, scorer=s).search(x), SE.PoseSearcher(g, receptor=rec, score_config=cfg, config=SEARCH).search(x))
    assert M.PoseMinimizer(g, scorer=s).scorer is s and SE.PoseSearcher(g, scorer=s).scorer is s
    for tool in (M.PoseMinimizer, SE.PoseSearcher):
        for extra in (dict(receptor=rec), dict(receptor="graph"), dict(score_config=cfg)):
            with pytest.raises(ValueError, match="scorer"):
                tool(g, scorer=s, **extra)
