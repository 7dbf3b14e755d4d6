"""sentence_transformers.losses: the pair, triplet, in-batch-negatives and batch-mining triplet objectives on the HIP path (st_losses.py)."""
from quadruplet_sentence_transformer_amd.st_losses import (BatchAllTripletLoss, BatchHardSoftMarginTripletLoss,  # noqa: F401
                                                           BatchHardTripletLoss, BatchHardTripletLossDistanceFunction,
                                                           BatchSemiHardTripletLoss, ContrastiveLoss, CosineSimilarityLoss,
                                                           MultipleNegativesRankingLoss,
                                                           MultipleNegativesSymmetricRankingLoss,
                                                           OnlineContrastiveLoss, SiameseDistanceMetric,
                                                           TripletDistanceMetric, TripletLoss)
