"""sentence_transformers.models: the Transformer / Pooling / Normalize descriptors that choose a head for a plain HF
checkpoint (SentenceTransformer(modules=[...])), and Dense, the trained projection head after pooling. Every other module
class of sentence-transformers is outside this build."""
from quadruplet_sentence_transformer_amd.models import Dense, Normalize, Pooling, Transformer  # noqa: F401
