from .base import Env, Wrapper, MaxStepWrapper, FrameStackWrapper, stack_sources
from .exp_sender_wrapper import (ExpSenderWrapperBase, ExpSenderWrapperSSAR,
                                 ExpSenderWrapperSSARNStepBootstrap,
                                 ExpSenderWrapperMultiStepMovingWindowWithInfo)
from .synthetic_env import SyntheticEnv, SyntheticVecEnv
from .adapters import (ObsTransform, GymAdapter, RobosuiteWrapper, DMControlAdapter, FilterWrapper,
                       ObservationConcatenationWrapper, TransposeWrapper, GrayscaleWrapper,
                       make_env, make_env_config, wrap_gym, wrap_robosuite, wrap_dm_control)
from .monitor import (EpisodeMonitor, ConsoleMonitor, TrainingTensorplexMonitor,
                      EvalTensorplexMonitor, DeviceEpisodeMonitor, DeviceTrainingMonitor, DeviceNoise,
                      DeviceParamNoise, DeviceEvaluator, DeviceEvalSnapshots)
from .device_recorder import DeviceWindowRecorder, DeviceNStepRecorder, closing_ranks
from .host_vec_env import HostVecEnv
