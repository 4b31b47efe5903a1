from .psrs import PSRS, BatchedPSRS, evalMC_psrs, evalmc_rollouts, qlearn_psrs, expSARSA_psrs, SHUFFLE_PER_ROLLOUT, SHUFFLE_SHARED, SHUFFLE_NONE  # noqa: F401
from .per_state_rejection import PerStateRejectionSampling  # noqa: F401
from .trivial_baselines import FollowObservationOnly, FollowActionOnly, ServeRandomTransitions  # noqa: F401
from .queue_evaluator import (QueueEvaluator, BatchedQueueEvaluator, evalmc_rollouts_queue, evalmc_rollouts_queue_population,  # noqa: F401
                              evalMC_queue, qlearn_queue, expSARSA_queue)
from .true_env_drivers import (GridWorld, BatchedGridWorld, evalMC_env, qlearn_env, expSARSA_env, rollout_env, evalmc_rollouts_env)  # noqa: F401
from .latent_env_drivers import (LatentEnv, BatchedLatentEnv, evalMC_latent_env, qlearn_latent_env, expSARSA_latent_env, z_expSARSA_env,  # noqa: F401
                                 evalmc_rollouts_latent_env)
from .psrs_exo import PSRS_Exo, BatchedPSRSExo, evalmc_rollouts_exo, tabulate_obs  # noqa: F401
from .vector_env import VectorPSRS  # noqa: F401
from .vector_queue import VectorQueueEvaluator  # noqa: F401
from .vector_true_env import VectorGridNavi, VectorCartPole  # noqa: F401
from .true_env_population import evalmc_rollouts_true_env  # noqa: F401
from .obs_policy import MLPPolicy, RowPolicy, CallablePolicy, MLPValue, RowValue, PolicyPopulation  # noqa: F401
from .batched import evalmc_rollouts_population  # noqa: F401
from .ppo_buffer import PPOBatch, ppo_advantages  # noqa: F401
from .ppo_learner import PPOLearner, PPOUpdateInfo, ppo_grad  # noqa: F401
from .ppo_population import PPOPopulation, ppo_grad_population  # noqa: F401
from .ppo_log import EpisodeTracker, PPOEpochLog, PPOEpisodes, PPOTrainLog, ppo_epoch_log, ppo_epoch_log_records  # noqa: F401
from .td_population import TDPopulation, TDPopulationResult  # noqa: F401
from .replay import ReplayLog, TDReplayResult, qlearn_replay, replay_orders, replay_td, replay_lpw  # noqa: F401
