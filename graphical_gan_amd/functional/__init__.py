"""torch.autograd bindings of the libggan C ABI.

torch supplies device memory, the current HIP stream and the autograd tape (the role tf.gradients plays in
the reference); every piece of arithmetic is a HIP kernel reached through include/ggan.h.  Each backward
is itself built from these Functions, so the gradient-penalty double backward works:
  conv_fwd'   = (conv_dgrad, conv_wgrad)        conv_dgrad' = (conv_fwd, conv_wgrad)
  conv_wgrad' = (conv_dgrad, conv_fwd)          gemm'       = (gemm, gemm)
There is no CPU path: tensors must live on a HIP device and libggan.so must load.
"""

# one module per op family (round-4 review: the 2 190-line functional.py split); this package re-exports every name, private helpers
# included, so that `from graphical_gan_amd import functional as F` reads as before
from ._core import (  # noqa: F401
    C, os, weakref, torch, Function, once_differentiable, _lib, ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH, ACT_SIGMOID, ConvGeom,
    check, _WS, _WS_BYTES, _L, _p, _stream, _dev, _c, _DEFER, _DATA_ONLY, _is_param, data_grad_only,
    _skip_undefined, defer_wgrad_reduce, _wgrad_parts, _STREAMS, shared_stream, workspace, _PLAN, _PLAIN, _SERIAL_BWD, target_workgroups,
    launch_hint, serial_backward, _remembers_plan, force_plain,
    same_geometry, conv_geom, _geom, _SITE, site_scope, site_plan, RowSlot, _new_out, _adjacent, HEAD_LOGITS, _PENDING_COSTS, _tail_value, settle_cost,
    pending_costs, drop_pending_costs, UNIT_SEEDS, unit_seed, is_unit_seed, LATE_EXT, _LATE_TERMS, mark_ready, wait_ready, add_late_terms,
    drop_late_terms)
from .pointwise import ActFwd, ActBwd, leaky_relu, relu, tanh, sigmoid  # noqa: F401
from .conv import (  # noqa: F401
    DEBUG_POISON_CHECK, PendingCast, ConvFwd, _fused_conv_backward, ConvDgrad, ConvDgradMasked, ConvWgrad, ChanSum, TALL_ROWS,
    ColSum)
from .linear import (  # noqa: F401
    Gemm, _fused_linear_backward, Gemm2, _CONSTS, cached_const, Gemm2Dgrad, HeadInputGrad, _HEAD_HINT, head_bce_hint, CriticHead, DynScan,
    gemm_colsum_, linear)
from .norm import BatchNormTrain, BatchNormGroupedTrain, BatchNormBwd, LinearBatchNormRows, _all_gather_rows, SyncBatchNormTrain  # noqa: F401
from .rows import (  # noqa: F401
    JoinRows, Fanout, fanout, SplitRows, CastScaleI32, Axpby, MixMean, GmmLatent, GmmLatentST, MixRbfMmd2, MixRbfMmd2Unbiased, mix_rbf_sums, mmd2_from_sums, MMD_FUSED_MAX_ROWS, knn_radii, ball_counts, prdc, PRDC_MAX_K, knn_lists, knn_vote, knn_accuracy, KNN_MAX_K, KNN_MAX_CLASSES, parzen_lse, parzen_ll, PARZEN_MAX_SIGMAS, ssim_pairs, psnr_from_mse, lsq_probe_fit, lsq_probe_predict, ProbeFit, PROBE_MAX_DIM, PROBE_MAX_CLASSES, PROBE_MAX_ROWS, PROBE_ROW_BLOCK, PROBE_BAD_LABEL, PROBE_NONFINITE, PROBE_BAD_PIVOT, lsq_probe_fit_wide, lsq_probe_predict_wide, WPROBE_MAX_DIM, WPROBE_TILE, WPROBE_PANEL, WPROBE_CHUNK, frechet_moments, frechet_distance, FRECHET_MAX_DIM, FRECHET_MAX_ROWS, FRECHET_NONFINITE, FRECHET_NOT_CONVERGED, sliced_wasserstein_projected, sliced_wasserstein, SWD_MAX_ROWS, SWD_MAX_DIRS, SWD_NONFINITE, Reparam, AGG_KL, AGG_IKL, AGG_JSD,
    AggDiv, RowLerp, gmm_posterior_assign_, cluster_accuracy_, sheet_grid, video_sheet_u8)
from .conv3d import _dims3, Im2Col3d, Col2Im3d, _conv3d_patch, _igemm_ok, Conv3dImplicit, conv3d  # noqa: F401
from .losses import BceSum, Distance, MeanSum, GradPenalty  # noqa: F401
from .losses import (  # noqa: F401
    SoftmaxXent, softmax_xent, class_score, ClassScore, CLS_MAX_CLASSES, CLS_MAX_SPLITS, CLS_MAX_BATCH, CLS_SCORE_MAX_ROWS, CLS_BAD_LABEL,
    CLS_NONFINITE)
from .kmeans import (  # noqa: F401
    kmeans_seed, kmeans_pick, kmeans_assign, kmeans_update, kmeans_fit, KMeansFit, bin_test, cluster_scores, KMEANS_MAX_K, KMEANS_MAX_CLASSES,
    KMEANS_ROW_BLOCK, KMEANS_MAX_ROWS, KMEANS_MAX_ITERS, KMEANS_NONFINITE, KMEANS_BAD_INDEX)
from .optim_ops import ema_step_, swap_  # noqa: F401
from .optim_ops import adam_step_, rmsprop_step_, NOISE_NORMAL, NOISE_UNIFORM, NOISE_ONEHOT, noise_state, noise_fill_, pack_  # noqa: F401
from .tsne import (  # noqa: F401
    tsne, tsne_splits, tsne_neighbours, tsne_affinities, tsne_symmetrise, tsne_gradient, tsne_kl, tsne_step, tsne_affinity_graph)
