"""guardx_amd -- MI355X-native batched GUARD environment step (gfx950 HIP kernels)
behind the guardX `safe_rl_envs` Engine interface."""
from .engine import Engine, ResamplingError  # noqa: F401
from .env_config import configuration, create_env  # noqa: F401
from .epstats import combine_episode_stats, constraint_value, episode_stats  # noqa: F401
from . import fisher  # noqa: F401
from .fisher import FisherOperator  # noqa: F401
from . import linesearch  # noqa: F401
from .linesearch import LineSearch  # noqa: F401
from . import vfit  # noqa: F401
from .vfit import ValueFit  # noqa: F401
from . import pgrad  # noqa: F401
from .pgrad import SurrogateGradient, cpo_direction, trpo_direction  # noqa: F401
from . import pifit  # noqa: F401
from .pifit import PolicyFit  # noqa: F401
from . import cfit  # noqa: F401
from .cfit import CostCriticFit  # noqa: F401

__version__ = "0.1.0"
