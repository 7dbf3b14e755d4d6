"""sentence_transformers.losses: the row-wise pair and triplet objectives on the HIP path (st_losses.py)."""
from quadruplet_sentence_transformer_amd.st_losses import (ContrastiveLoss, CosineSimilarityLoss,  # noqa: F401
                                                           OnlineContrastiveLoss, SiameseDistanceMetric,
                                                           TripletDistanceMetric, TripletLoss)
