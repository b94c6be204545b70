"""Learner-side glue that consumes the env's outputs: A2C loss with the return scan on the GPU, and a
preallocated trajectory buffer — same class names as the reference's `wurm.rl` — and the fused A2C learner of the
feed-forward agent (loss, backward pass, clip and Adam in HIP), for one agent or a population of them, with the training
statistics of the fused loops (RolloutStats, MultiRolloutStats: the reference's log columns, kept on the device) and the
per-policy results of a league (LeagueTable)."""
from wurm_amd.rl.a2c import A2C, a2c_returns
from wurm_amd.rl.fused_learner import FusedA2CLearner
from wurm_amd.rl.fused_population import FusedA2CPopulation
from wurm_amd.rl.league_table import LeagueTable
from wurm_amd.rl.multi_rollout_stats import MultiRolloutStats
from wurm_amd.rl.rollout_stats import RolloutStats
from wurm_amd.rl.trajectory_store import TrajectoryStore

__all__ = ['A2C', 'a2c_returns', 'FusedA2CLearner', 'FusedA2CPopulation', 'LeagueTable', 'MultiRolloutStats', 'RolloutStats',
           'TrajectoryStore']
