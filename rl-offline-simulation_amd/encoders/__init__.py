from .heuristic import CartpoleBoxEncoder  # noqa: F401
from .homer import HOMEREncoder  # noqa: F401
from .homer_population import HOMERPopulation, epoch_draws  # noqa: F401
