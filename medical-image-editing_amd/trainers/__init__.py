from .first_step import FirstStepTrainer, FlipViews, RandomTransformViews, LossWeights  # noqa: F401
from .data_parallel import GradientAllReducer  # noqa: F401
from .second_step import SecondStepTrainer, GanLossWeights  # noqa: F401
from .second_step_unet import UNetSecondStepTrainer, UNetGanLossWeights, draw_cutmix_box  # noqa: F401
from .second_step_unet_mw import UNetMultiWindowSecondStepTrainer  # noqa: F401
from .vqgan_unet_dis import VQGANUNetDisTrainer, VQGANLossWeights  # noqa: F401
from .config import (build_first_step_trainer, build_second_step_trainer, build_vqgan_trainer, check_vqgan_config, vqgan_loss_weights, configure_discriminator, configure_vqgan, gan_loss_weights, unet_gan_loss_weights, configure_models, configure_optimizers, configure_losses, configure_frequency_loss,  # noqa: F401
                     configure_perceptual_loss,
                     loss_weights, set_transform, build_evaluator)
from .config import build_prior_trainer, check_prior_config, check_edit_config, check_detect_config, configure_prior  # noqa: F401
from .config import check_synth_config, guidance, prior_cond_drop, prior_condition  # noqa: F401
from .prior import PriorTrainer, learning_rate, parameter_groups  # noqa: F401
from .cond_prior import ConditionalPriorTrainer  # noqa: F401
from .masked_prior import MaskedPriorTrainer  # noqa: F401
from .masked_cond_prior import ConditionalMaskedPriorTrainer  # noqa: F401
from .config import prior_masked, edit_n_steps, synth_n_steps  # noqa: F401
from .config import detect_pseudo, edit_pnll  # noqa: F401
from .config import detect_lesionwise  # noqa: F401
from .config import blend, check_blend, default_blend_levels  # noqa: F401
from .evaluation import Evaluator, write_result_csv  # noqa: F401
from .fit import Fit, InferenceModels, build_loader  # noqa: F401
