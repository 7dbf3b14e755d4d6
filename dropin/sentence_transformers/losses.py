"""sentence_transformers.losses: the pair, triplet and in-batch-negatives objectives on the HIP path (st_losses.py)."""
from quadruplet_sentence_transformer_amd.st_losses import (ContrastiveLoss, CosineSimilarityLoss,  # noqa: F401
                                                           MultipleNegativesRankingLoss,
                                                           MultipleNegativesSymmetricRankingLoss,
                                                           OnlineContrastiveLoss, SiameseDistanceMetric,
                                                           TripletDistanceMetric, TripletLoss)
