from quadruplet_sentence_transformer_amd.evaluation import (EmbeddingSimilarityEvaluator,  # noqa: F401
                                                            InformationRetrievalEvaluator, ParaphraseMiningEvaluator,
                                                            QuadrupletEvaluator,
                                                            QuadrupletLossEvaluator, SentenceEvaluator,
                                                            SequentialEvaluator, SimilarityFunction, TripletEvaluator,
                                                            get_sequential_evaluator)
