from quadruplet_sentence_transformer_amd.evaluation import (EmbeddingSimilarityEvaluator,  # noqa: F401
                                                            InformationRetrievalEvaluator, LabelAccuracyEvaluator,
                                                            MSEEvaluator,
                                                            ParaphraseMiningEvaluator,
                                                            QuadrupletEvaluator,
                                                            QuadrupletLossEvaluator, SentenceEvaluator,
                                                            SequentialEvaluator, SimilarityFunction, TranslationEvaluator,
                                                            TripletEvaluator,
                                                            get_sequential_evaluator)
