"""ctgcn_amd — MI355X-native CTGCN embedding engine: the hot path in HIP, and the reference's config-driven driver over it
(train.gnn_embedding, baseline.dyngem_embedding, preprocessing.preprocess, `python -m ctgcn_amd.main`).

The sparse aggregation of CoreDiffusion over nested k-core adjacency matrices and the k-core peel that
produces them run as hand-written HIP kernels for gfx950 behind a C ABI (include/ctgcn_hip.h,
ctgcn_amd/csrc/libctgcn_hip.so); this package is the host-side mirror of the reference's interface for that
path: layers.CoreDiffusion, models.{CDN,CGCN,CTGCN}, helper.DataLoader.get_core_adj_list,
preprocessing.StructureInfoGenerator.  There is no CPU fallback.
"""
from ._lib import CtgcnHipError  # noqa: F401
from .core_adj import CoreAdj  # noqa: F401
from .layers import CoreDiffusion, MLP  # noqa: F401
from .models import CDN, CGCN, CTGCN, EdgeClassifier, InnerProduct, MLPClassifier  # noqa: F401
from .helper import DataLoader  # noqa: F401
from .metrics import (ClassificationLoss, NegativeSamplingLoss, ReconstructionLoss, StructureClassificationLoss, VAEClassificationLoss,  # noqa: F401
                      VAELoss)
from .embedding import SupervisedEmbedding, UnsupervisedEmbedding  # noqa: F401
from .baseline import (GAT, GCN, GCRN, GIN, PGNN, SAGE, Aggregator, EvolveGCN, GraphConvolution, Nonlinear, PGNN_layer,  # noqa: F401
                       SAGE_Layer, SpGraphAttentionLayer, VGRNN, GCNConv, InnerProductDecoder, graph_gru_gcn, BatchGenerator, BatchPredictor,
                       DynAE, DynamicEmbedding, DynGraph2VecLoss, RegularizationLoss, DynGEM, DynGEMBatchGenerator, DynGEMBatchPredictor,
                       DynGEMLoss, DynRNN, DynAERNN, MLLSTM, MTMLP, TIMERS, timers, timers_embedding, dyngem_embedding, TgGAT, TgGATConv, TgGCN, TgGCNConv, TgGIN,
                       TgGINConv, TgSAGE, TgSAGEConv)
from .train import gnn_embedding, window_schedule  # noqa: F401
from .evaluation import DataGenerator, LinkPredictor, aggregate_results, evaluate, evaluate_window, link_prediction  # noqa: F401

__all__ = ["CtgcnHipError", "CoreAdj", "CoreDiffusion", "MLP", "CDN", "CGCN", "CTGCN", "DataLoader", "NegativeSamplingLoss", "ReconstructionLoss",
           "UnsupervisedEmbedding", "SupervisedEmbedding", "MLPClassifier", "InnerProduct", "EdgeClassifier", "ClassificationLoss",
           "StructureClassificationLoss", "DataGenerator", "LinkPredictor", "aggregate_results", "evaluate", "evaluate_window", "link_prediction", "EvolveGCN",
           "GCN", "GraphConvolution", "GCRN", "GAT", "SpGraphAttentionLayer", "GIN", "SAGE", "SAGE_Layer", "Aggregator", "PGNN", "PGNN_layer", "Nonlinear",
           "VGRNN", "GCNConv", "graph_gru_gcn", "InnerProductDecoder", "VAELoss", "VAEClassificationLoss",
           "DynAE", "RegularizationLoss", "DynGraph2VecLoss", "BatchGenerator", "BatchPredictor", "DynamicEmbedding", "DynGEM", "DynGEMLoss",
           "DynGEMBatchGenerator", "DynGEMBatchPredictor", "DynRNN", "DynAERNN", "MLLSTM", "MTMLP",
           "TIMERS", "timers", "timers_embedding", "dyngem_embedding", "gnn_embedding", "window_schedule",
           "TgGCN", "TgGAT", "TgSAGE", "TgGIN", "TgGCNConv", "TgGATConv", "TgSAGEConv", "TgGINConv"]
