"""Evaluation of trained embeddings.  link_prediction: the reference's evaluation/link_prediction.py on the GPU (ctgcn_eval.hip);
centrality_prediction: its evaluation/centrality_prediction.py (ctgcn_cent.hip); node_classification: its
evaluation/node_classification.py (ctgcn_nodecls.hip); edge_classification: its evaluation/edge_classification.py (the pair-gather
passes of ctgcn_nodecls.hip); similarity_prediction: its evaluation/similarity_prediction.py (ctgcn_sim.hip); graph_reconstruction:
this package's own MAP / precision@k over a ranking of all node pairs (ctgcn_topk.hip)."""
from .link_prediction import (DataGenerator, LinkPredictor, aggregate_results, evaluate, evaluate_window,  # noqa: F401
                              link_prediction, make_splits)
from ._logreg import FitReport, roc_auc  # noqa: F401
from .centrality_prediction import (CentralityPredictor, PowerIterationFailedConvergence, centralities,  # noqa: F401
                                    centrality_prediction, ridge_cv_errors)
from .centrality_prediction import DataGenerator as CentralityDataGenerator  # noqa: F401
from .centrality_prediction import evaluate as evaluate_centrality  # noqa: F401
from .node_classification import (NodeClassifier, evaluate_window as evaluate_node_classification_window,  # noqa: F401
                                  node_classification)
from .node_classification import DataGenerator as NodeClsDataGenerator  # noqa: F401
from .node_classification import aggregate_results as aggregate_node_classification_results  # noqa: F401
from .node_classification import evaluate as evaluate_node_classification  # noqa: F401
from .edge_classification import (EdgeClassifier, evaluate_window as evaluate_edge_classification_window,  # noqa: F401
                                  edge_classification)
from .edge_classification import DataGenerator as EdgeClsDataGenerator  # noqa: F401
from .edge_classification import aggregate_results as aggregate_edge_classification_results  # noqa: F401
from .edge_classification import evaluate as evaluate_edge_classification  # noqa: F401
from .similarity_prediction import (SimilarityPredictor, similarity_prediction, spearman, vertex_similarity)  # noqa: F401
from .similarity_prediction import DataGenerator as SimilarityDataGenerator  # noqa: F401
from .similarity_prediction import evaluate as evaluate_similarity  # noqa: F401
from .graph_reconstruction import GraphReconstructor, graph_reconstruction  # noqa: F401
from .graph_reconstruction import evaluate as evaluate_graph_reconstruction  # noqa: F401
