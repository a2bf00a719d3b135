"""MI355X-native vectorised RIS-VEC environment (hot path of 20242204033/RIS-VEC-MARL's
`Simulation-MARL-BCD/Environment.py`), behind the reference's `Environ` class surface.

    from ris_vec_marl_amd import Environ, VecEnviron, apply_yaml_config

All computation runs in hand-written HIP kernels (csrc/, C ABI in include/risvec.h);
importing the package does not need a GPU, computing does.
"""
from .params import EnvParams, apply_yaml_config, load_yaml, reference_lanes, poisson_cdf_table
from .vec_env import VecEnviron
from .compat import Environ, Vehicle, encode_noma_groups
from .sarl import OUNoise, SarlEnviron, SarlParams, SarlReplayBuffer, sarl_action_map, sarl_observe
from .noma import NomaConfig, NomaGrouper, anneal_topk
from .replay import VecReplayBuffer, marshal_actions
from .policy import BatchedPolicy
from .actor import BatchedActor, pack_actor_weights_device
from .critic import (BatchedCritic, ddpg_soft_update, ddpg_td_target, pack_critic_weights, pack_critic_weights_device,
                     unpack_critic_weights)
from .marl_critic import (BatchedTwinCritic, pack_marl_critic_weights, pack_marl_critic_weights_device,
                          pack_marl_critic_weights_wide_device)
from .local_critics import BatchedLocalCritics
from .optim import BatchedAdam
from .metrics import EpisodeMeter, ScalarSink
from . import dist

__all__ = ["EnvParams", "apply_yaml_config", "load_yaml", "reference_lanes", "poisson_cdf_table",
           "VecEnviron", "Environ", "Vehicle", "encode_noma_groups", "SarlEnviron", "SarlParams", "sarl_action_map",
           "sarl_observe", "OUNoise", "SarlReplayBuffer", "NomaConfig", "NomaGrouper", "anneal_topk", "VecReplayBuffer",
           "marshal_actions", "BatchedPolicy", "BatchedActor", "pack_actor_weights_device", "BatchedCritic",
           "ddpg_td_target", "ddpg_soft_update", "pack_critic_weights", "pack_critic_weights_device", "unpack_critic_weights", "BatchedTwinCritic",
           "pack_marl_critic_weights", "pack_marl_critic_weights_device", "pack_marl_critic_weights_wide_device",
           "BatchedLocalCritics", "BatchedAdam", "EpisodeMeter", "ScalarSink", "dist"]
