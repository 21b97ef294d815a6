"""
coot-videotext_amd: MI355X (gfx950) implementation of the COOT retrieval training hot path
(simon-ging/coot-videotext: coot/model_retrieval.py, coot/loss_fn.py, coot/trainer_retrieval.py
hooks, nntrainer/models/*) as hand-written HIP kernels behind a C ABI (include/coot_hip.h).
"""
from . import lib  # noqa: F401
from . import synthetic  # noqa: F401
from .config import (RetrievalConfig, RetrievalNetworksConst, TransformerConfig, TransformerTypesConst,  # noqa: F401
                     load_named_config, load_yaml_config_file)
from .loss_fn import (ContrastiveLoss, ContrastiveLossConfig, cycle_consistency_loss, sample_cycle_indices,  # noqa: F401
                      total_contrastive_loss)
from .model_retrieval import (RetrievalDataBatchTuple, RetrievalModelManager, RetrievalTextEmbTuple,  # noqa: F401
                              RetrievalVisualEmbTuple, RetrievalPackedBatchTuple, attach_packed_index, packed_index)
from .nets import TransformerHip, pack_by_count  # noqa: F401
from .retrieval import (RETRIEVAL_FEW_MAX, GalleryIndex, compute_retrieval, compute_retrieval_cosine, compute_retrieval_counts_part,  # noqa: F401
                        compute_retrieval_labeled, compute_retrieval_labeled_device, compute_retrieval_range, compute_retrieval_topk,
                        compute_retrieval_topk_grouped, compute_retrieval_self_join, retrieval_self_join_device,
                        compute_retrieval_components, retrieval_components_device,
                        compute_retrieval_join, retrieval_join_device, compute_retrieval_knn_join, retrieval_knn_join_device,
                        compute_retrieval_topk_masked, compute_retrieval_topk_multi, compute_retrieval_topk_scoped, retrieval_metrics_device,
                        retrieval_range_device, retrieval_ranks_labeled_device, retrieval_ranks_part_device, retrieval_topk_device, retrieval_topk_grouped_device,
                        retrieval_topk_index_device, retrieval_topk_multi_device, retrieval_topk_scoped_device,
                        compute_retrieval_topk_adjusted, compute_retrieval_hub_offsets, retrieval_topk_adjusted_device,
                        compute_retrieval_labeled_adjusted, retrieval_ranks_adjusted_device, compute_retrieval_adjusted_device,
                        compute_retrieval_csls_device)
from .trainer_retrieval import GradClip, LossScaler, RetrievalTrainer, make_optimizer  # noqa: F401
from .validation import loader_order_permutation, save_embeddings, shard_batch_indices  # noqa: F401
from . import lr_scheduler  # noqa: F401,E402
from .dataset_retrieval import BatchArena, DeviceLoader, RetrievalDataPointTuple, collate_fn  # noqa: F401,E402
