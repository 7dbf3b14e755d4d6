"""sentence_transformers.losses: the pair, triplet, in-batch-negatives, batch-mining triplet, distillation (pairwise and
over a list of candidates: DistillKLDivLoss), softmax-classifier and pairwise-ranking (CoSENT, AnglE) objectives on the HIP path, MatryoshkaLoss over them, the
GradCache forms of the in-batch-negatives losses, and GISTEmbedLoss with its GradCache form (st_losses.py)."""
from quadruplet_sentence_transformer_amd.st_losses import (AnglELoss, BatchAllTripletLoss, BatchHardSoftMarginTripletLoss,  # noqa: F401
                                                           BatchHardTripletLoss, BatchHardTripletLossDistanceFunction,
                                                           BatchSemiHardTripletLoss, CachedGISTEmbedLoss,
                                                           CachedMultipleNegativesRankingLoss,
                                                           CachedMultipleNegativesSymmetricRankingLoss, ContrastiveLoss,
                                                           CoSENTLoss,
                                                           CosineSimilarityLoss, DistillKLDivLoss, GISTEmbedLoss,
                                                           MarginMSELoss, MatryoshkaLoss, MSELoss,
                                                           MultipleNegativesRankingLoss,
                                                           MultipleNegativesSymmetricRankingLoss,
                                                           OnlineContrastiveLoss, SiameseDistanceMetric, SoftmaxLoss,
                                                           TripletDistanceMetric, TripletLoss)
