"""diffdock_pocket_amd - MI355X-native (gfx950) drop-in for DiffDock-Pocket's reverse-diffusion score-model
hot path.  See DESIGN.md for the scope, include/ddp_hip.h for the C ABI and INTEGRATION.md for how the reference
binds to it."""
from .batch import HeteroBatch, Store, collate, set_time  # noqa: F401
from .diffusion import SigmaRanges, get_t_schedule, get_timestep_embedding, sinusoidal_embedding, t_to_sigma  # noqa: F401

__all__ = ["HeteroBatch", "Store", "collate", "set_time", "SigmaRanges", "get_t_schedule", "get_timestep_embedding",
           "sinusoidal_embedding", "t_to_sigma", "get_model", "TensorProductScoreModel", "PoseEvaluator", "PoseClusters", "summarize", "PoseRefiner",
           "RefineConfig", "RefineResult", "PoseScorer", "ScoreConfig", "PoseScores", "PoseMinimizer", "MinimizeConfig",
           "MinimizeResult", "FlexPoseMinimizer", "FlexMinimizeResult", "InteractionProfiler", "ProfileConfig", "InteractionProfile",
           "PoseSearcher", "SearchConfig", "SearchResult", "FlexPoseSearcher", "FlexSearchResult"]


def __getattr__(name):  # lazy: importing the model pulls in torch.nn and the ctypes binding
    if name == "TensorProductScoreModel":
        from .score_model import TensorProductScoreModel
        return TensorProductScoreModel
    if name == "get_model":
        from .factory import get_model
        return get_model
    if name in ("PoseEvaluator", "PoseClusters", "summarize"):
        from . import evaluation
        return getattr(evaluation, name)
    if name in ("PoseRefiner", "RefineConfig", "RefineResult"):
        from . import refine
        return getattr(refine, name)
    if name in ("PoseScorer", "ScoreConfig", "PoseScores"):
        from . import scoring
        return getattr(scoring, name)
    if name in ("PoseMinimizer", "MinimizeConfig", "MinimizeResult"):
        from . import minimize
        return getattr(minimize, name)
    if name in ("FlexPoseMinimizer", "FlexMinimizeResult"):
        from . import minimize_flex
        return getattr(minimize_flex, name)
    if name in ("InteractionProfiler", "ProfileConfig", "InteractionProfile"):
        from . import interactions
        return getattr(interactions, name)
    if name in ("PoseSearcher", "SearchConfig", "SearchResult"):
        from . import search
        return getattr(search, name)
    if name in ("FlexPoseSearcher", "FlexSearchResult"):
        from . import search_flex
        return getattr(search_flex, name)
    raise AttributeError(name)
