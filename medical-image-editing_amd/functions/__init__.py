"""Drop-in `functions` package (reference: functions/__init__.py): losses of the first training step."""
from .embed_loss import EmbeddingLoss  # noqa: F401
from .onehot import OneHotEncoder  # noqa: F401
from .seg_loss import SoftDiceLoss, FocalLoss  # noqa: F401
from .gan_loss import hinge_d_loss, generator_loss  # noqa: F401
from .freq_loss import FocalFrequencyLoss  # noqa: F401
from .perceptual_loss import VGGLoss  # noqa: F401
from .lpips_loss import LPIPSLoss  # noqa: F401
from .metrics import MeanSquaredError, StructuralSimilarityIndexMeasure, PeakSignalNoiseRatio, label_entropy  # noqa: F401
from .sample_scores import FeatureStats, Moments, frechet_distance, manifold_scores, code_scores, sample_scores  # noqa: F401
from .lesion_scores import LesionScores, derived_scores, lesion_csv_row, LESION_SCORES, LESION_CSV  # noqa: F401
