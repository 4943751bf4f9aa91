"""``vited_amd.engine`` is a package of one module per concern; its callers still reach everything as ``engine.X``."""
from vited_amd import engine

# what ``engine`` exported when it was one module: every name defined there without a leading underscore, and the one private
# helper the tests use
SURFACE = [
    'ClassificationMeters', 'DevicePrefetcher', 'Div2kDeviceLoader', 'Div2kImageStore', 'FlatGradients', 'GeshaemMetrics',
    'HISFRAG_PLAN_COLUMNS', 'HisfragDeviceLoader', 'HisfragPlan', 'MICHIGAN_MAX_HOLES', 'MICHIGAN_PLAN_COLUMNS', 'MeterValue',
    'MichiganDeviceLoader', 'MichiganPlan', 'MinedPairs', 'NativeScalerWithGradNormCount', 'PUZZLE_SIDES', 'PairScoreAggregator',
    'PairScoreStats', 'PuzzleCompatibility', 'PuzzleSolution', 'TrainMeters', 'TrainStep', 'ValidationResult', 'assemble_pairs',
    'broadcast_parameters', 'build_optimizer', 'class_members', 'configure_ddp', 'div2k_augment_plan', 'div2k_pair_plan',
    'geshaem_pair_metrics', 'group_relations', 'hisfrag_augment_plan', 'hisfrag_feed', 'hisfrag_prepare_data',
    'hisfrag_prepare_indexed', 'hisfrag_prepare_mined', 'hisfrag_retrieval_metrics', 'map_prak', 'metrics_from_sums',
    'michigan_augment_plan', 'michigan_feed', 'mine_pairs', 'mine_pairs_device', 'mined_bce_with_logits', 'mined_pair_capacity',
    'pair_relevancy', 'pairwise_similarity', 'param_groups_no_decay_1d', 'puzzle_accuracy', 'puzzle_distances',
    'relevancy_from_cams', 'retrieval_metrics', 'shard_rows_by_pair_count', 'solve_puzzle', 'validate_classifier',
    '_decoder_only_parameters',
]

HOMES = {'TrainStep': 'train', 'FlatGradients': 'distributed', 'MichiganDeviceLoader': 'feeds', 'mine_pairs_device': 'mining',
         'pairwise_similarity': 'similarity', 'map_prak': 'metrics', 'solve_puzzle': 'puzzle', 'pair_relevancy': 'relevancy'}


def test_every_name_is_still_an_attribute_of_engine():
    missing = [name for name in SURFACE if not hasattr(engine, name)]
    assert not missing, missing


def test_reexports_are_the_objects_of_their_modules():
    for name, module in HOMES.items():
        assert getattr(engine, name) is getattr(getattr(engine, module), name), (name, module)


def test_michigan_loader_only_names_its_plan_and_feed():
    own = vars(engine.MichiganDeviceLoader)
    assert 'plan' not in own and '__iter__' not in own
