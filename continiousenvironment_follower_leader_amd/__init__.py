"""MI355X-native batched ``Game.step()`` for the continuous_grid_arctic follow-the-leader env."""
from . import abi  # noqa: F401
from .config import make_config, GameConfig  # noqa: F401


def __getattr__(name):
    # ScenarioSampler lives beside VecGame (vec_game.py imports torch): looked up on first use
    if name == "ScenarioSampler":
        from .vec_game import ScenarioSampler
        return ScenarioSampler
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
