from quadruplet_sentence_transformer_amd.evaluation import (EmbeddingSimilarityEvaluator,  # noqa: F401
                                                            InformationRetrievalEvaluator,
                                                            SentenceEvaluator, SequentialEvaluator,
                                                            SimilarityFunction, TripletEvaluator)
