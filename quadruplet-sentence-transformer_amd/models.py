"""The module descriptors of sentence-transformers 2.2.2 that pick a head for a plain HF checkpoint:

    SentenceTransformer(modules=[models.Transformer("bert-base-uncased", max_seq_length=256),
                                 models.Pooling(768, pooling_mode="cls"), models.Normalize()])

They hold settings only and compute nothing: SentenceTransformer(modules=...) reads them into an EncoderConfig and runs the
whole chain in libqst.so. The chain Transformer -> Pooling -> [Normalize] is the only one accepted; `dropin/` re-exports
this module as `sentence_transformers.models`.
"""
from __future__ import annotations

from typing import Optional

from .config import POOLING_MODES, pooling_modes

# ST 2.2.2 Pooling config keys (1_Pooling/config.json, in the order ST writes them) -> mode names of config.POOLING_MODES
POOLING_CONFIG_KEYS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean",
                       "pooling_mode_max_tokens": "max", "pooling_mode_mean_sqrt_len_tokens": "mean_sqrt_len",
                       "pooling_mode_weightedmean_tokens": "weightedmean"}


class Transformer:
    """sentence_transformers.models.Transformer: the HF checkpoint (a local directory or a model name resolved offline)
    and its max_seq_length (None: the checkpoint's own, at most 512)."""

    def __init__(self, model_name_or_path: str, max_seq_length: Optional[int] = None, model_args: Optional[dict] = None,
                 cache_dir: Optional[str] = None, tokenizer_args: Optional[dict] = None, do_lower_case: bool = False,
                 tokenizer_name_or_path: Optional[str] = None):
        self.model_name_or_path = model_name_or_path
        self.max_seq_length = max_seq_length
        self.cache_dir = cache_dir
        self.do_lower_case = do_lower_case
        if tokenizer_name_or_path not in (None, model_name_or_path):
            raise NotImplementedError("a tokenizer from another directory than the model's is not supported")


class Pooling:
    """sentence_transformers.models.Pooling: pooling_mode ("cls", "max", "mean", "mean_sqrt_len", "weightedmean" or a
    '+' join of them) or the pooling_mode_*_tokens flags, as in ST 2.2.2 (a pooling_mode string overrides the flags).
    `pooling` is the mode string of config.EncoderConfig, in the fixed block order."""

    def __init__(self, word_embedding_dimension: int, pooling_mode: Optional[str] = None,
                 pooling_mode_cls_token: bool = False, pooling_mode_max_tokens: bool = False,
                 pooling_mode_mean_tokens: bool = True, pooling_mode_mean_sqrt_len_tokens: bool = False,
                 pooling_mode_weightedmean_tokens: bool = False, pooling_mode_lasttoken: bool = False):
        self.word_embedding_dimension = int(word_embedding_dimension)
        if pooling_mode is not None:
            if str(pooling_mode).lower() == "lasttoken":
                raise NotImplementedError("pooling_mode='lasttoken' is not implemented (cls, max, mean, mean_sqrt_len, "
                                          "weightedmean)")
            modes = pooling_modes(str(pooling_mode).lower())
        else:
            if pooling_mode_lasttoken:
                raise NotImplementedError("pooling_mode_lasttoken is not implemented (cls, max, mean, mean_sqrt_len, "
                                          "weightedmean)")
            flags = {"cls": pooling_mode_cls_token, "max": pooling_mode_max_tokens, "mean": pooling_mode_mean_tokens,
                     "mean_sqrt_len": pooling_mode_mean_sqrt_len_tokens, "weightedmean": pooling_mode_weightedmean_tokens}
            modes = tuple(m for m in POOLING_MODES if flags[m])
            if not modes:
                raise ValueError("Pooling: no pooling mode enabled")
        self.pooling = "+".join(modes)

    def get_pooling_mode_str(self) -> str:
        return self.pooling

    def get_sentence_embedding_dimension(self) -> int:
        return len(pooling_modes(self.pooling)) * self.word_embedding_dimension

    def get_config_dict(self) -> dict:
        """1_Pooling/config.json as ST 2.2.2 writes it."""
        on = set(pooling_modes(self.pooling))
        out = {"word_embedding_dimension": self.word_embedding_dimension}
        out.update({k: m in on for k, m in POOLING_CONFIG_KEYS.items()})
        out["pooling_mode_lasttoken"] = False
        return out


class Normalize:
    """sentence_transformers.models.Normalize: L2-normalise the pooled vector (over all of its D columns)."""


def pooling_from_config(pool: dict, hidden_size: int, where: str = "") -> str:
    """The pooling string of a 1_Pooling/config.json. An enabled mode other than the five of POOLING_MODES (lasttoken, or
    any key a later sentence-transformers writes), no enabled mode, or a word_embedding_dimension other than hidden_size
    is refused: the checkpoint would be pooled wrongly."""
    pre = f"{where}: " if where else ""
    bad = sorted(k for k, v in pool.items() if k.startswith("pooling_mode") and v and k not in POOLING_CONFIG_KEYS)
    if bad:
        raise NotImplementedError(f"{pre}pooling {bad} is not implemented (cls, max, mean, mean_sqrt_len, weightedmean); "
                                  "this checkpoint would be pooled wrongly")
    on = set(m for k, m in POOLING_CONFIG_KEYS.items() if pool.get(k))
    if not on:
        raise NotImplementedError(f"{pre}no pooling mode enabled in {sorted(pool)}")
    dim = pool.get("word_embedding_dimension", hidden_size)
    if int(dim) != int(hidden_size):
        raise NotImplementedError(f"{pre}Pooling word_embedding_dimension {dim} differs from the encoder's hidden_size "
                                  f"{hidden_size}")
    return "+".join(m for m in POOLING_MODES if m in on)
