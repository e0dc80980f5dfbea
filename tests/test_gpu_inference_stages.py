"""The device twin of tests/test_inference_stages_cpu.py: the stages of one row on device tensors, in their fused forms, give the same
bits from one shared _RowTools (one scorer and its device tables behind the scoring, the minimiser and the searcher, one receptor
behind the rest) as from tools built separately for each stage.  Every kernel behind them sums in a fixed order without atomics, so
the equality is exact.  No kernel is new here: what is pinned is the sharing of the device tables."""
import os

import pytest
import torch

from diffdock_pocket_amd import evaluation as EV
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import interactions as IA
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd import scoring as SC
from test_evaluation_cpu import GOLDEN, graph_3dpf
from test_inference_stages_cpu import MIN, SEARCH, same
from test_scoring_cpu import fixture_3dpf, perturbed_poses

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("flex", [False, True])
def test_the_stages_of_one_shared_row_equal_separately_built_ones_on_the_device(flex):
    dev = _dev()
    g, pdb, _ = fixture_3dpf()
    if flex:
        g = graph_3dpf("A:160-A:193-A:197")[0]
    with open(os.path.join(GOLDEN, "3dpf_ligand.sdf")) as f:
        texts = (pdb, f.read())
    lig = perturbed_poses()[:3].to(dev)
    apos = g["atom"].pos.float()[None].repeat(3, 1, 1).to(dev) if flex else None
    cfg = SC.ScoreConfig()

    def tools():
        return INF._RowTools({"complex_name": "3dpf"}, g, dev, flex, cfg, texts)

    stages = {"score": lambda t: t.score(lig, apos).cpu(), "minimize": lambda t: t.minimize(lig, apos, MIN),
              "search": lambda t: t.search(lig, apos, SEARCH), "evaluate": lambda t: t.evaluate(lig, apos),
              "cluster": lambda t: t.cluster(lig, 2.0), "refine": lambda t: t.refine(lig, apos, R.RefineConfig(iterations=3), True),
              "interactions": lambda t: t.interactions(lig, apos, IA.ProfileConfig(), True)}
    shared = tools()
    for name, run in stages.items():
        got, want = run(shared), run(tools())
        torch.cuda.synchronize()
        for a, b in zip(got, want) if isinstance(got, tuple) else ((got, want),):
            same(a, b, name)
    assert shared.scorer._dev["rec"].is_cuda and shared.scorer.receptor_from_graph == flex


def test_device_poses_are_refused_by_host_tools_in_the_words_always_used():
    dev = _dev()
    g, _, rec = fixture_3dpf()
    lig = perturbed_poses()[:2].to(dev)
    for who, entry in (("scorer", SC.PoseScorer(g, receptor=rec).score), ("refiner", R.PoseRefiner(g).refine),
                       ("profiler", IA.InteractionProfiler(g).profile), ("evaluator", EV.PoseEvaluator(g).evaluate),
                       ("evaluator", EV.PoseEvaluator(g).contacts)):
        with pytest.raises(ValueError) as e:
            entry(lig)
        assert str(e.value) == f"poses on {dev}, {who} built for cpu"
