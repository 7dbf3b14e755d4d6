"""sentence_transformers.datasets: the loaders the in-batch-negatives and the batch-mining triplet losses are documented
with (data.py)."""
from quadruplet_sentence_transformer_amd.data import NoDuplicatesDataLoader, SentenceLabelDataset  # noqa: F401
