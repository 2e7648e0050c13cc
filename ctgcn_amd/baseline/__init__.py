"""Methods CTGCN is compared against (the reference's `baseline` package), on the same HIP library."""
from .dynae import BatchGenerator, BatchPredictor, DynAE, DynamicEmbedding, DynGraph2VecLoss, RegularizationLoss, dyngem_embedding  # noqa: F401  (its MLP: baseline.dynae.MLP)
from .dyngem import DynGEM, DynGEMBatchGenerator, DynGEMBatchPredictor, DynGEMLoss  # noqa: F401
from .dynrnn import MLLSTM, DynRNN  # noqa: F401
from .dynaernn import MTMLP, DynAERNN  # noqa: F401
from .egcn import EvolveGCN  # noqa: F401
from .gat import GAT, SpGraphAttentionLayer  # noqa: F401
from .gcn import GCN, GraphConvolution  # noqa: F401
from .gcrn import GCRN  # noqa: F401
from .gin import GIN  # noqa: F401
from .pgnn import (PGNN, Nonlinear, PGNN_layer, anchor_set_count, get_dist_max, get_random_anchorset,  # noqa: F401
                   precompute_dist_data, preselect_anchor)
from .sage import SAGE, SAGE_Layer, Aggregator  # noqa: F401
from .tg import TgGAT, TgGATConv, TgGCN, TgGCNConv, TgGIN, TgGINConv, TgSAGE, TgSAGEConv  # noqa: F401
from .timers import TIMERS, timers, timers_embedding  # noqa: F401
from .vgrnn import VGRNN, GCNConv, InnerProductDecoder, LazyInnerProduct, gcn_conv_adjacency, graph_gru_gcn  # noqa: F401
