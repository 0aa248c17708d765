from .loss import (NCELearnableTempDSLLoss, NCELearnableTempLoss, NCELearnableTempLoss_vs_vc,  # noqa: F401
                   NCELearnableTempLoss_vs_vc_fc, NCELearnableTempLoss_vsc, NCELearnableTempLoss_vsc_fc,
                   VidImgDivideNCELearnableTempLoss, VidImgNCELearnableTempLoss, build_loss_func)
from .adamw import AdamW  # noqa: F401
from .sched import get_lr_sched  # noqa: F401
from .utils import build_e2e_optimizer_w_lr_mul, setup_e2e_optimizer  # noqa: F401
