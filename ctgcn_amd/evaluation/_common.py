"""What the five evaluation tasks share on the host: the GPU-or-raise helpers, the reference's file conventions (node file, embedding
files, the walk over a method's snapshots), the choice of C and the avg / max / min columns of the aggregated tables.  `task` is the
name an error message speaks of ("link-prediction", ...)."""
import os

import pandas as pd
import torch

from ..utils import read_edge_rows


def device(device, task):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("%s evaluation needs a ROCm GPU: no CPU fallback" % task)
    return torch.device("cuda", torch.cuda.current_device())


def require_cuda(t, what, task):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (ROCm) tensor: %s evaluation runs on the GPU, no CPU fallback" % (what, task))


def stream(dev=None):
    return torch.cuda.current_stream(dev).cuda_stream


def read_nodes(path):
    return pd.read_csv(path, names=['node'])['node'].tolist()


def read_embedding(path, sep, full_node_list, dtype=None):
    """The rows of an embedding file in node-file order (numpy [n, d]; cast to dtype when given)."""
    values = pd.read_csv(path, sep=sep, index_col=0).loc[full_node_list].values
    return values if dtype is None else values.astype(dtype)


def select_C(val_scores):
    """Index of the best validation score; the reference compares with >=, so the last of tied values wins."""
    best, idx = 0, -1
    for i, a in enumerate(val_scores):
        if a >= best:
            best, idx = a, i
    return idx


def snapshot_rows(file_path, full_node_list, sep, note=''):
    """(src, dst, weight) of a snapshot file's rows as indices into full_node_list.  A node missing from it raises ValueError
    (`note` is added to its text)."""
    node2idx = dict(zip([str(v) for v in full_node_list], range(len(full_node_list))))
    try:
        return read_edge_rows(file_path, node2idx, sep)
    except KeyError as e:
        raise ValueError("%s names a node that is not in the node file%s: %s" % (file_path, note, e))


def method_snapshots(origin_path, embedding_path, method, lag=0, first=None):
    """(date, file name, embedding path) of every snapshot file of origin_path, in sorted order, whose embedding under
    embedding_path/method exists; lag = 1 pairs a snapshot with the embedding of the one before it (and skips the first).
    first(date), when given, reads the snapshot's own data and its result is yielded as a fourth item: like the reference it runs
    before the embedding is looked for, so a missing data file raises even where the snapshot would be skipped."""
    f_list = sorted(os.listdir(origin_path))
    for i, f_name in enumerate(f_list[lag:], lag):
        date = f_name.split('.')[0]
        own = (first(date),) if first else ()
        path = os.path.join(embedding_path, method, f_list[i - lag])
        if os.path.exists(path):
            yield (date, f_name, path) + own


def aggregate_stats(df, cols):
    """Append the avg, max and min over the columns `cols` of every row."""
    df['avg'] = df.loc[:, cols].mean(axis=1)
    df['max'] = df.loc[:, cols].max(axis=1)
    df['min'] = df.loc[:, cols].min(axis=1)
    return df
