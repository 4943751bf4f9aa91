"""What drives the model on MI355X, re-plumbed from the reference's trainers (misc/engine.py, misc/utils.py, hisfrag.py,
michigan.py, evaluation.py, main.py): one process per GPU, RCCL all-reduce of a single flat fp32 gradient buffer over xGMI
instead of c10d's 25 MB DDP buckets, bf16 autocast instead of fp16 + GradScaler, the forward + backward replayable as hipGraphs,
and the input pipelines and evaluation paths on the device; loading from disk, logging and checkpoints stay in the reference.

One concern per module: ``distributed`` (process group, flat gradient exchange), ``train`` (optimizer, ``TrainStep``, meters),
``feeds`` (prefetcher; DIV2K, HisFrag, Michigan and Pajigsaw device loaders, evaluation sources), ``mining`` (pair mining and its loss), ``similarity`` (the
streamed similarity matrix), ``metrics`` (retrieval, group mAP / Pr@k, geshaem, classifier validation), ``puzzle`` (with ``puzzle_mixed``), ``relevancy``,
``lr_finder`` (the learning-rate range test).
Every public name is re-exported here, so callers write ``engine.TrainStep``.  State that is rebound at run time is not: read
and set ``engine.train._CAPTURE_MODE`` there."""
from .distributed import FlatGradients, broadcast_parameters, configure_ddp  # noqa: F401
from .feeds import (HISFRAG_PLAN_COLUMNS, MICHIGAN_MAX_HOLES, MICHIGAN_PLAN_COLUMNS, CenterCropSource, DevicePrefetcher,  # noqa: F401
                    Div2kDeviceLoader, Div2kImageStore, HisfragDeviceLoader, HisfragPlan, MichiganDeviceLoader, MichiganEvalSource,
                    MichiganPlan, PajigsawDeviceLoader, PajigsawIndex, assemble_pairs, div2k_augment_plan, div2k_pair_plan,
                    hisfrag_augment_plan, hisfrag_feed, michigan_augment_plan, michigan_feed, pajigsaw_index, pajigsaw_pair_plan,
                    pajigsaw_pieces, resize_images)
from .lr_finder import LR_FINDER_MAX_ITER, LRFinderResult, LRRangeTest, find_lr  # noqa: F401
from .metrics import (ClassificationMeters, GeshaemMetrics, MeterValue, PairScoreAggregator, PairScoreStats, RetrievalCurves,  # noqa: F401
                      RetrievalLists, ValidationResult, class_members, geshaem_pair_metrics, group_relations,
                      hisfrag_retrieval_lists, hisfrag_retrieval_metrics, map_prak, metrics_from_sums, retrieval_curves,
                      retrieval_metrics, retrieval_topk, validate_classifier)
from .mining import (MinedPairs, hisfrag_prepare_data, hisfrag_prepare_indexed, hisfrag_prepare_mined, mine_pairs,  # noqa: F401
                     mine_pairs_device, mined_bce_fused, mined_bce_with_logits, mined_pair_capacity)
from .puzzle import (PUZZLE_SIDES, PuzzleCompatibility, PuzzleCut, PuzzleSolution, cut_puzzle, puzzle_accuracy,  # noqa: F401
                     puzzle_distances, puzzle_model_pieces, puzzle_pixel_distances, reconstruct_puzzle, solve_model_puzzle, solve_pixel_puzzle,
                     solve_puzzle)
from .puzzle_mixed import PuzzleBoards  # noqa: F401
from .relevancy import pair_relevancy, relevancy_from_cams  # noqa: F401
from .similarity import pairwise_similarity, shard_rows_by_pair_count  # noqa: F401
from .train import (NativeScalerWithGradNormCount, TrainMeters, TrainStep, TwoStageTrainStep, _decoder_only_parameters,  # noqa: F401
                    build_optimizer, build_scheduler, param_groups_no_decay_1d)
