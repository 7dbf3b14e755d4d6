from quadruplet_sentence_transformer_amd.evaluation import (BinaryClassificationEvaluator,  # noqa: F401
                                                            EmbeddingSimilarityEvaluator,
                                                            InformationRetrievalEvaluator, LabelAccuracyEvaluator,
                                                            MSEEvaluator,
                                                            ParaphraseMiningEvaluator,
                                                            QuadrupletEvaluator,
                                                            QuadrupletLossEvaluator, RerankingEvaluator, SentenceEvaluator,
                                                            SequentialEvaluator, SimilarityFunction, TranslationEvaluator,
                                                            TripletEvaluator,
                                                            get_sequential_evaluator)
