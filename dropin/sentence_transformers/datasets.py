"""sentence_transformers.datasets: the loaders the in-batch-negatives and the batch-mining triplet losses are documented
with, and the parallel-sentence dataset of the distillation recipe (data.py)."""
from quadruplet_sentence_transformer_amd.data import (NoDuplicatesDataLoader, ParallelSentencesDataset,  # noqa: F401
                                                      SentenceLabelDataset)
