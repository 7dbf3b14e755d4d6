"""Drop-in `sentence_transformers` namespace for the reference's unchanged scripts: put `<repo>/dropin` (and the
repo root) on PYTHONPATH ahead of site-packages and `from sentence_transformers import SentenceTransformer,
InputExample` resolves to the MI355X-native implementation."""
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)

from quadruplet_sentence_transformer_amd.sentence_transformer import InputExample, SentenceTransformer  # noqa: E402,F401
from . import util, evaluation, models  # noqa: E402,F401


class CrossEncoder:
    """Placeholder for sentence_transformers.CrossEncoder. The reference builds one at import time
    (models/evaluators.py:31, a remote fetch of "cross-encoder/stsb-roberta-large") and only uses it when the IR
    evaluation set is filtered with --use_cross_encoder. Cross-encoders are outside this build (SURVEY.md 8f rank 2:
    "make CrossEncoder optional/offline"): construction succeeds so the module imports, scoring refuses."""

    def __init__(self, model_name: str = "", *args, **kwargs):
        self.model_name = model_name

    def predict(self, *args, **kwargs):
        raise RuntimeError(f"CrossEncoder({self.model_name!r}).predict: cross-encoder scoring is not part of the "
                           "MI355X-native build (no pretrained weights offline); build the IR evaluation set with "
                           "use_cross_encoder=False")

__version__ = "2.2.2+qst_amd"
