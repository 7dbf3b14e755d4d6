"""sentence_transformers.cross_encoder: the HIP CrossEncoder (quadruplet_sentence_transformer_amd.cross_encoder)."""
from quadruplet_sentence_transformer_amd.cross_encoder import CrossEncoder  # noqa: F401
