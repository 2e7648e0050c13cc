"""Evaluation of trained embeddings.  link_prediction: the reference's evaluation/link_prediction.py on the GPU (ctgcn_eval.hip)."""
from .link_prediction import (DataGenerator, LinkPredictor, aggregate_results, evaluate, evaluate_window,  # noqa: F401
                              link_prediction, make_splits)
from ._logreg import FitReport, roc_auc  # noqa: F401
