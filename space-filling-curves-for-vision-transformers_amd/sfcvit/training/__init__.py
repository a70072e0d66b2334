from .optim import FlatGradBuffer, FusedAdamW, WarmupCosine, WarmupCosineScheduler  # noqa: F401
from .train import AccumSteps, GraphedTrainStep, SoftTargetCrossEntropy, mixup_soft_targets, train_step  # noqa: F401
from .distributed import GradReducer  # noqa: F401
from .mix import BatchMix  # noqa: F401
from .augment import DeviceAugment  # noqa: F401
