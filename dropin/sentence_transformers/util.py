from quadruplet_sentence_transformer_amd.util import (batch_to_device, community_detection, cos_sim, dot_score,  # noqa: F401
                                                      euclidean_score, hamming_topk, int8_topk, mine_hard_negatives, paraphrase_mining,
                                                      pairwise_angle_sim, pairwise_cos_sim, pairwise_dot_score,
                                                      paraphrase_mining_embeddings, pytorch_cos_sim, semantic_search,
                                                      topk_merge_rows, topk_rows, topk_scores, topk_stream)
