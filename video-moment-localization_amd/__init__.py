"""MI355X-native SMIN hot path (cross-modal fusion + 2D temporal proposal scoring).

Drop-in for the ``models.py`` module surface of ChanukyaVardhan/Video-Moment-Localization:
same classes, constructor/forward signatures and state_dict keys, with the
per-cell work done by hand-written HIP kernels for gfx950 behind the C ABI in
``include/smin_hip.h`` (``libsmin_hip.so``, bound with ctypes in ``_lib.py``).

The directory name contains '-' so it cannot be imported by name; the repo-root ``models.py``
loads it under the module name ``vml_amd``.
"""
from . import _lib, distributed  # noqa: F401,E402
from ._lib import get_gemm_mode, set_gemm_mode  # noqa: F401
from .cells import CellLayout  # noqa: F401
from .modules import (  # noqa: F401
    SMIN, SMI, Attention, Backbone, BoundaryUnit, ContentAttention, ContentUnit, Localization,
    MomentUnit, ProposalGeneration, QueryEncoder, VideoEncoder, compute_content_matrix, VideoBank, QueryBank,
)
from .training import loss_fn, loss_fn_torch, bce_loss, compute_ious, compute_ious_torch, CapturedStep  # noqa: F401
from .training import train_epoch, eval_epoch, test_model, test_model_windows, test_model_corpus, test_model_corpus_windows  # noqa: F401
from .training import test_model_corpus_window_shards  # noqa: F401
from .training import search_shards_weighted, search_window_shards_weighted  # noqa: F401
from .training import test_model_corpus_weighted_shards, test_model_corpus_window_shards_weighted  # noqa: F401
from .training import pair_targets, train_epoch_pairs, train_epoch_mined, pair_rank_loss, pair_rank_loss_torch  # noqa: F401
from .training import prefilter_rank_loss, train_epoch_prefilter  # noqa: F401
from .training import pair_distill_loss, pair_distill_loss_torch, prefilter_distill_loss  # noqa: F401
from .training import search_shards_prefiltered, test_model_corpus_prefiltered_shards  # noqa: F401
from .retrieval import PairPlan, SurvivorBank, WindowBank  # noqa: F401
from .meter import EpochMeter, EpochMeterTorch, CorpusMeter, CorpusMeterTorch, VideoRankMeter, CutFidelityMeter  # noqa: F401
from .optim import FusedAdam, FusedAdamTorch, RowSparseAdam, RowSparseAdamTorch  # noqa: F401
from .labels import build_targets  # noqa: F401
from .moments import top_moments, top_moments_torch, top_moments_soft_torch, merge_window_moments, merge_window_moments_torch  # noqa: F401
from .moments import corpus_span_topk, corpus_span_topk_torch, merge_search_windows, merge_search_windows_torch  # noqa: F401
from .moments import corpus_topk, corpus_topk_torch, merge_search, merge_search_torch, mine_pairs, mine_pairs_torch  # noqa: F401
from .moments import pair_pool, pair_pool_torch, group_pool, group_pool_torch, rank_videos, rank_videos_torch  # noqa: F401
from .moments import reweight_moments, reweight_moments_torch  # noqa: F401
from .moments import prefilter_scores, prefilter_scores_torch, prefilter_select, prefilter_select_torch, prefilter_maps  # noqa: F401
from .moments import expand_survivor_windows, expand_survivor_windows_torch, survivor_window_capacity  # noqa: F401
from .moments import prefilter_fold, prefilter_fold_torch, survivors_admit, survivors_admit_torch, prefilter_gt_rank, prefilter_gt_rank_torch  # noqa: F401
from .moments import bank_encode, bank_encode_torch, bank_decode, bank_decode_torch, BANK_STORAGES  # noqa: F401
from .moments import merge_search_weighted, merge_search_weighted_torch  # noqa: F401
from .moments import merge_search_windows_weighted, merge_search_windows_weighted_torch  # noqa: F401
from .moments import span_ious, span_ious_torch, compute_span_ious, compute_span_ious_torch  # noqa: F401
from .feeder import BatchFeeder, FedBatch, build_targets_hip, build_masks_hip, cell_count  # noqa: F401
from .sampling import (  # noqa: F401
    sample_clips, sample_clips_torch, embed_tokens, embed_tokens_torch, RowSparseGrad, merge_row_grads, merge_row_grads_torch,
    clip_indices, draw_offsets, spos_high,
    window_plan, sample_windows, sample_windows_torch, window_annotations, draw_windows,
)
