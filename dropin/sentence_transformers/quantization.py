from quadruplet_sentence_transformer_amd.quantization import (column_ranges, hamming_topk, int8_topk,  # noqa: F401
                                                              quantize_embeddings, rescore_quantized,
                                                              semantic_search_quantized)
