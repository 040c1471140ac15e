"""MI355X-native distribution-distance engine behind the audio-metrics API.

Importable as ``audio_metrics_amd`` (the directory name carries a hyphen; the
top-level ``audio_metrics_amd/`` shim points Python at it).
"""
from . import _lib, hip_ops                        # noqa: F401
from ._build import build_library, LIB_PATH        # noqa: F401

from .data import AudioMetricsData, ensure_tensor, ensure_ndarray            # noqa: F401
from . import metrics                                                         # noqa: F401
from .metrics.fad import frechet_distance, frechet_distance_inf               # noqa: F401
from .metrics.fad import frechet_distance_per_group                           # noqa: F401
from .metrics.fad_stats import frechet_distance_with_error, frechet_distance_compare   # noqa: F401
from .metrics.fad_stats import frechet_standard_error, frechet_difference_test       # noqa: F401
from .metrics.kd import kernel_distance, kid_features_to_metric               # noqa: F401
from .metrics.kad import kernel_audio_distance                                # noqa: F401
from .metrics.kad import kernel_audio_distance_per_group                      # noqa: F401
from .metrics.kad_stats import kernel_audio_distance_with_error              # noqa: F401
from .metrics.kad_stats import kernel_audio_distance_compare                  # noqa: F401
from .metrics.kad_stats import mmd_standard_error, mmd_difference_test        # noqa: F401
from .metrics.kad_perm import kernel_audio_distance_permutation_test, mmd_permutation_null   # noqa: F401
from .metrics.mmd import kernel_audio_distance_multiscale, energy_distance   # noqa: F401
from .metrics.prdc import prdc, nearest_neighbour_distances                   # noqa: F401
from .metrics.neighbors import nearest_neighbors                              # noqa: F401
from .metrics.fidelity import sample_fidelity, sample_fidelity_per_group, fidelity_by_group   # noqa: F401
from .metrics.prdc_groups import leave_group_out_radii, prdc_leave_group_out    # noqa: F401
from .metrics.pprecall import probabilistic_precision_recall, probabilistic_precision_per_group   # noqa: F401
from .metrics.pprecall import psr_radius, psr_by_group                        # noqa: F401
from .metrics.mauve import kmeans, mauve_score, mauve_from_histograms         # noqa: F401
from .metrics.sinkhorn import sinkhorn_divergence, sinkhorn_schedule       # noqa: F401
from .metrics.sliced import sliced_wasserstein_distance, sliced_directions   # noqa: F401
from .metrics.classifier import (inception_score, inception_score_per_group, kl_divergence_paired,   # noqa: F401
                                 paired_cosine_score)
from .metrics.apa import apa, apa_compute_d_x_xp                              # noqa: F401
from .metrics.vendi import vendi_score, vendi_score_per_group, vendi_from_eigenvalues   # noqa: F401
from .metrics.fkea import (vendi_score_rff, rke_score, kernel_novelty_score, rff_frequencies,   # noqa: F401
                           novelty_from_eigenvalues)
from .metrics.fld import (feature_likelihood_divergence, feature_likelihood_fit, fld_adam_step,   # noqa: F401
                          fld_from_logliks, authenticity_score)
from .metrics.c2st import classifier_two_sample_test, c2st_folds, c2st_summary, logistic_lbfgs   # noqa: F401
from .metrics.nn_test import nearest_neighbor_two_sample_test, nn_permutation_null   # noqa: F401
from .metrics.dependence import (distance_correlation, kernel_alignment, dependence_from_sums,   # noqa: F401
                                 dependence_permutations, row_dependence, dcor_t_test)
from .metrics.retrieval import retrieval_scores, retrieval_summary            # noqa: F401

from .embed import ItemCategory, embedding_pipeline                            # noqa: F401
from .projection import IncrementalPCA                                         # noqa: F401
from .audio_metrics import AudioMetrics                                        # noqa: F401

__version__ = "0.1.0"
