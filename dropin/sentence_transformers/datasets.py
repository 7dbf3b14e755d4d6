"""sentence_transformers.datasets: the loader the in-batch-negatives losses are documented with (data.py)."""
from quadruplet_sentence_transformer_amd.data import NoDuplicatesDataLoader  # noqa: F401
