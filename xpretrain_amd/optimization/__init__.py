from .loss import (HardNegLoss, MILNCEContrastiveLoss, NCEContrastiveLoss, TripletContrastiveLoss,  # noqa: F401
                   NCELearnableTempDSLLoss, NCELearnableTempLoss, NCELearnableTempLoss_vs_vc,
                   NCELearnableTempLoss_vs_vc_fc, NCELearnableTempLoss_vsc, NCELearnableTempLoss_vsc_fc,
                   VidImgDivideNCELearnableTempLoss, VidImgNCELearnableTempLoss, build_loss_func)
from .adam import Adam, Adamax  # noqa: F401
from .adamw import AdamW  # noqa: F401
from .sched import get_lr_sched  # noqa: F401
from .utils import build_e2e_optimizer_w_lr_mul, setup_e2e_optimizer  # noqa: F401
