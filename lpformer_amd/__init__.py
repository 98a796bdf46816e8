"""lpformer_amd -- MI355X-native LPFormer link-scoring forward pass (hand-written gfx950 HIP behind a C ABI).

Public surface mirrors the reference (HarryShomer/LPFormer):
    LinkTransformer, mlp_score          drop-ins for src/models/link_transformer.py / other_models.py
    LPFormer                            torch_geometric.nn.models.LPFormer-style facade (logits out)
    calc_ppr, calc_ppr_gpu, get_ppr     drop-ins for src/util/calc_ppr_scores.py (host OpenMP push / MI355X push)
    evaluate                            encoder-once, device-resident evaluation sweep + ranking metrics (also by bin);
                                        rank_counts / ranks / sample_hits / link_metrics / split_metrics /
                                        evaluate_model: ranks, Hits@K, MRR, AUC, AP from device rank-count kernels
    pair_heuristics                     CN / Adamic-Adar / Resource Allocation (+ PPR, feature cosine) of pairs
    pair_distance, DIST_BINS            shortest-path hops per pair (device bidirectional BFS) and its bins for
                                        metrics_by_bin / attention_profile
    pair_walks, pair_katz               walk counts (A^l)[a, b], l <= 4, per pair (device meet-in-the-middle kernel) and
                                        the truncated Katz index; katz_from_walks, walks_reference (numpy restatement)
    pair_hop_counts                     nodes by distance to both endpoints, int32 [P, k+2, k+2] per pair, k <= 2
                                        (device spread-and-expand kernel): what there was to select, per node class;
                                        elph_features (the ELPH / BUDDY layout), ball_jaccard, hop_counts_reference
                                        (numpy restatement)
    node_structure                      degree, core number, component (smallest id) and triangle count of every node
                                        (device h-index sweeps, hook-and-jump, sorted-row intersection): NodeStructure
                                        (clustering, component_size, summary), pair_node_values / same_component (the
                                        per-pair axis for metrics_by_bin), DEGREE_BINS, CORE_BINS, structure_reference
                                        (numpy / scipy restatement)
    communities                         Louvain communities of the typing adjacency (device move rounds: short rows in
                                        registers, hub rows through an LDS hash table; exact integers, a pure function
                                        of graph and seed): Communities (label = smallest id, size, hierarchy, summary),
                                        same_community / COMMUNITY_BINS (intra- or inter-community, for metrics_by_bin),
                                        partition_quality (exact modularity numerator of any labelling),
                                        communities_reference (numpy restatement)
    recommend                           top-K new links per source node (device candidates, scoring, top-K)
    similar_nodes                      the m nodes nearest to each query by inner product or cosine over the encoder's
                                        output, the raw features or any table (device matrix-core kernel with the top-m
                                        kept in LDS: no [S, n] matrix); Similar, similar_reference (numpy restatement)
    explain, explain_from_scores        per-pair attention attribution: top nodes, mass per type, entropy (device
                                        segmented reduction); pairs_of (a recommend result's pairs), attention_profile
    threshold_profile, suggest_thresholds   selected-node counts per pair, type and PPR threshold for a whole grid of
                                        thresholds in one device pass; the grid triple that fits an entry budget
    heart_negatives, twohop_rows        HeaRT-style hard negatives [P, K, 2] made on the device; rows of A diag(w) A
    update_ppr, update_data, update_graph   graph edits with an exact incremental PPR refresh (ppr_affected_sources)
    TrainEdges, train_epoch, fit        the training epoch: the reference's per-batch edge mask made exactly on the
                                        device (repeated pairs included), the loop, and epochs with early stopping
    negative_rows, negative_pairs       uniform negatives that avoid known edges, drawn on the device: K targets per
                                        source / M distinct pairs; UniformNegatives (fresh non-edges per training step
                                        for train_epoch(negatives=...)), negatives_reference (numpy restatement)
    bootstrap_metrics, compare_metrics  standard errors, percentile intervals and paired p-values of Hits@K / MRR / AUC by
                                        a bootstrap over the positives (device resampling kernel); bootstrap_by_bin,
                                        bootstrap_sums (the building block), bootstrap_sums_reference (numpy restatement)
    random_walks, node2vec_embeddings   node2vec's biased second-order walks drawn on the device (rejection sampling with
                                        exact integer thresholds: a pure function of seed and walk id): Walks (walks,
                                        forced), walk_thresholds, walk_pairs (skip-gram pairs as PyG cuts them), and the
                                        Node2Vec embeddings trained on them (skip-gram in torch); the numpy restatement
                                        is random_walks.walks_reference
    skipgram_step, skipgram_state       one Node2Vec skip-gram step with negative sampling on the device (PyG's loss,
                                        SparseAdam; three kernels, one summation order, repeatable bits): what
                                        node2vec_embeddings(trainer="device") runs; SkipGramState, skipgram_reference
                                        (the fp64 restatement on the CPU)
    cn_pool, NCNPredictor               the sum of a table's rows over each pair's common neighbours (device fused
                                        intersect-and-gather kernel, one summation order, differentiable in the table)
                                        and NCN's predictor on it -- LPFormer with uniform attention on the common
                                        neighbours only; cn_entries (the common neighbours themselves), ncn_scores,
                                        cn_pool_reference / cn_entries_reference (the fp64 / numpy restatements)
    link_split                          edge list + features -> a data dict with train / valid / test positives and
                                        edge-aware negatives, ready for fit and evaluate_model
    graph, data                         CSR containers and the data-dict builder
"""
from . import evaluate, graph, mask_delta, readers  # noqa: F401
from .bootstrap import (bootstrap_by_bin, bootstrap_metrics, bootstrap_sums, bootstrap_sums_reference,  # noqa: F401
                        compare_metrics)
from .community import (COMMUNITY_BINS, Communities, communities, communities_reference,  # noqa: F401
                        partition_quality, same_community)
from .data import link_split  # noqa: F401
from .distance import DIST_BINS, pair_distance  # noqa: F401
from .epoch import TrainEdges, fit, train_epoch  # noqa: F401
from .explain import Explanation, attention_profile, explain, explain_from_scores, pairs_of  # noqa: F401
from .graph import RemovedEdges  # noqa: F401
from .graph_update import ppr_affected_sources, update_data, update_graph, update_ppr  # noqa: F401
from .hard_negatives import HardNegatives, heart_negatives, twohop_rows  # noqa: F401
from .heuristics import pair_heuristics  # noqa: F401
from .hops import ball_jaccard, elph_features, hop_counts_reference, pair_hop_counts  # noqa: F401
from .katz import katz_from_walks, pair_katz, pair_walks, walks_reference  # noqa: F401
from .ncn import (CnEntries, NCNPredictor, cn_entries, cn_entries_reference, cn_pool,  # noqa: F401
                  cn_pool_reference, ncn_scores)
from .negatives import UniformNegatives, negative_pairs, negative_rows, negatives_reference  # noqa: F401
from .graphed import GraphedScorer, PlannedScorer  # noqa: F401
from .link_transformer import MLP, LinkTransformer, mlp_score  # noqa: F401
from .ppr import calc_ppr, calc_ppr_gpu, get_ppr, load_or_calc_ppr, ppr_coo  # noqa: F401
from .pyg_api import LPFormer  # noqa: F401
from .random_walks import Walks, node2vec_embeddings, random_walks, walk_pairs, walk_thresholds  # noqa: F401
from .skipgram import SkipGramState, skipgram_reference, skipgram_state, skipgram_step  # noqa: F401
from .recommend import Recommendations, recommend  # noqa: F401
from .similar import Similar, similar_nodes, similar_reference  # noqa: F401
from .structure import (CORE_BINS, DEGREE_BINS, NodeStructure, node_structure, pair_node_values,  # noqa: F401
                        same_component, structure_reference)
from .threshold_profile import ThresholdProfile, suggest_thresholds, threshold_profile  # noqa: F401

__all__ = ["LinkTransformer", "mlp_score", "MLP", "LPFormer", "calc_ppr", "calc_ppr_gpu", "get_ppr",
           "load_or_calc_ppr", "ppr_coo", "graph", "evaluate", "GraphedScorer", "PlannedScorer", "RemovedEdges",
           "pair_heuristics", "recommend", "Recommendations", "heart_negatives", "twohop_rows",
           "HardNegatives", "ppr_affected_sources", "update_ppr", "update_data", "update_graph", "explain", "explain_from_scores",
           "pairs_of", "attention_profile", "Explanation", "threshold_profile", "suggest_thresholds", "ThresholdProfile",
           "TrainEdges", "train_epoch", "fit", "pair_distance", "DIST_BINS", "pair_walks",
           "pair_katz", "katz_from_walks", "walks_reference", "negative_rows", "negative_pairs", "UniformNegatives",
           "negatives_reference", "link_split", "pair_hop_counts", "hop_counts_reference", "elph_features",
           "ball_jaccard", "bootstrap_sums", "bootstrap_sums_reference", "bootstrap_metrics", "compare_metrics",
           "bootstrap_by_bin", "similar_nodes", "similar_reference", "Similar", "node_structure", "NodeStructure",
           "structure_reference", "pair_node_values", "same_component", "DEGREE_BINS", "CORE_BINS", "communities",
           "Communities", "communities_reference", "partition_quality", "same_community", "COMMUNITY_BINS", "random_walks",
           "node2vec_embeddings", "walk_pairs", "walk_thresholds", "Walks", "SkipGramState", "skipgram_state",
           "skipgram_step", "skipgram_reference", "cn_pool", "cn_entries", "cn_pool_reference", "cn_entries_reference",
           "CnEntries", "NCNPredictor", "ncn_scores"]
