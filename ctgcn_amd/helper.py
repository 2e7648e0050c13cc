"""DataLoader with the reference's constructor and get_core_adj_list signature (reference helper.py:12-82),
returning one CoreAdj per snapshot instead of K torch sparse tensors per snapshot.

get_core_adj_list reads the per-k .npz files the reference's preprocessing writes
(<core_base_path>/<snapshot>/<kk>.npz, scipy CSR, N x N).  get_core_adj_list_from_graphs is the native route:
it never materialises per-k files — snapshot edge lists go to the GPU, the HIP k-core peel tags every edge
with its level, and the loader semantics are applied through a level -> slot table.
"""
import os

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .core_adj import CoreAdj
from .utils import get_sp_adj_mat, read_edge_rows


class DataLoader(object):
    def __init__(self, node_list, max_time_num, has_cuda=False):
        self.max_time_num = max_time_num
        self.full_node_list = node_list
        self.node_num = len(node_list)
        self.node2idx_dict = dict(zip(node_list, np.arange(self.node_num)))
        self.has_cuda = has_cuda

    @property
    def device(self):
        return torch.device('cuda') if self.has_cuda else torch.device('cpu')

    def _window(self, start_idx, duration):
        return range(start_idx, min(start_idx + duration, self.max_time_num))

    # ----------------------------------------------------------------------------- .npz route
    def get_core_adj_list(self, core_base_path, start_idx, duration, max_core=-1):
        """list[T] of CoreAdj (len(CoreAdj) == K_t).  Loader rules kept bit for bit (reference helper.py:51-82):
        snapshots and files visited in sorted() order; max_core == -1 becomes the first visited snapshot's file
        count and STAYS that for the rest of the window; files 1..max_core are kept and visited from the
        largest k down; the first gets + I; a later matrix equal in sum to its predecessor is dropped."""
        date_dirs = sorted(os.listdir(core_base_path))
        assert start_idx < len(date_dirs)
        from .preprocessing.structure_generation import CACHE_SUFFIX
        if date_dirs and all(d.endswith(CACHE_SUFFIX) for d in date_dirs):
            return self.get_core_adj_list_from_cache(core_base_path, start_idx, duration, max_core)
        window = []
        for i in self._window(start_idx, duration):
            folder = os.path.join(core_base_path, date_dirs[i])
            names = sorted(os.listdir(folder))
            if max_core == -1:
                max_core = len(names)
            chosen = names[:max_core][::-1]
            kept, prev = [], None
            for j, name in enumerate(chosen):
                mat = sp.load_npz(os.path.join(folder, name))
                if j > 0 and (mat - prev).sum() == 0:
                    prev = mat
                    continue
                prev = mat
                kept.append(mat)
            if not kept:
                window.append([])       # snapshot without edges: the reference also yields an empty list
                continue
            adj = CoreAdj.from_nested_matrices_device(kept, self.device, self_loop=True) if self.has_cuda else None
            window.append(adj if adj is not None else CoreAdj.from_matrices(kept, self_loop=True, device=self.device))
        return window

    # -------------------------------------------------------------------------- native route
    def get_core_adj_list_from_graphs(self, origin_base_path, start_idx, duration, max_core=-1, sep='\t',
                                      return_core_numbers=False):
        """Same result as preprocessing (structure_generation.py) followed by get_core_adj_list, computed on
        the GPU straight from the snapshot edge lists under origin_base_path."""
        if not self.has_cuda:
            raise RuntimeError("the native route runs the HIP k-core peel: construct DataLoader(has_cuda=True)")
        files = sorted(os.listdir(origin_base_path))
        assert start_idx < len(files)
        window, cores = [], []
        for i in self._window(start_idx, duration):
            src, dst, w = read_edge_rows(os.path.join(origin_base_path, files[i]), self.node2idx_dict, sep)
            adj, core, file_count = core_adj_from_edge_rows(src, dst, w, self.node_num, max_core, self.device)
            if max_core == -1:
                max_core = file_count
            window.append(adj if adj is not None else [])
            cores.append(core)
        return (window, cores) if return_core_numbers else window

    def get_core_adj_list_from_cache(self, cache_base_path, start_idx, duration, max_core=-1, return_core_numbers=False):
        """Same result as get_core_adj_list on the per-k files, read from one <snapshot>.coreadj.npz per snapshot (written by
        StructureInfoGenerator(..., cache_folder=...)): the CSR and the stored core numbers go to the GPU, the k-core
        matrices become a level -> slot table — no peel, no per-k files, any max_core from the same file."""
        if not self.has_cuda:
            raise RuntimeError("the cache route builds the tagged CSR on the GPU: construct DataLoader(has_cuda=True)")
        from .preprocessing.structure_generation import read_core_cache
        files = sorted(os.listdir(cache_base_path))
        assert start_idx < len(files)
        window, cores = [], []
        for i in self._window(start_idx, duration):
            indptr, indices, data, core = read_core_cache(os.path.join(cache_base_path, files[i]))
            row_ptr = torch.from_numpy(indptr).to(self.device)
            col = torch.from_numpy(indices).to(self.device)
            val = torch.from_numpy(data.astype(np.float32)).to(self.device)
            adj, core_t, file_count = CoreAdj.from_graph(row_ptr, col, val, max_core=max_core, core=torch.from_numpy(core).to(self.device))
            if max_core == -1:
                max_core = file_count
            window.append(adj if adj is not None else [])
            cores.append(core_t)
        return (window, cores) if return_core_numbers else window

    # ------------------------------------------------------------ negative-sampling inputs (helper.py:26-49)
    def get_node_pair_list(self, walk_pair_base_path, start_idx, duration):
        """Per snapshot the co-occurrence partners of every node, read from the reference's `<snapshot>.npz` files, as
        device-resident WalkPairs (list-like: len() == N, [i] -> partner list)."""
        from .walks import WalkPairs
        files = sorted(os.listdir(walk_pair_base_path))
        out = []
        for i in self._window(start_idx, duration):
            m = sp.load_npz(os.path.join(walk_pair_base_path, files[i])).tocsr()
            m.sort_indices()
            out.append(WalkPairs(torch.from_numpy(m.indptr.astype(np.int32)).to(self.device),
                                 torch.from_numpy(m.indices.astype(np.int32)).to(self.device)))
        return out

    def get_node_freq_list(self, node_freq_base_path, start_idx, duration):
        """Per snapshot the negative table (`<snapshot>.json`), as an int32 tensor on the loader's device."""
        import json
        files = sorted(os.listdir(node_freq_base_path))
        out = []
        for i in self._window(start_idx, duration):
            with open(os.path.join(node_freq_base_path, files[i]), 'r') as fp:
                out.append(torch.tensor(json.load(fp), dtype=torch.int32, device=self.device))
        return out

    # ------------------------------------------------------------ supervised labels (helper.py:194-222)
    def _label_list(self, base_path, start_idx, duration, sep, node_cols):
        import pandas as pd
        files = sorted(os.listdir(base_path))
        out, seen = [], set()
        names = ['node', 'label'] if node_cols == 1 else ['from_id', 'to_id', 'label']
        for i in self._window(start_idx, duration):
            df = pd.read_csv(os.path.join(base_path, files[i]), sep=sep, header=0, names=names)
            for col in names[:node_cols]:
                df[col] = df[col].map(lambda x: self.node2idx_dict[x])
            seen.update(df['label'].unique().tolist())
            out.append(torch.from_numpy(df.values.astype(np.int64)).to(self.device))
        return out, len(seen)

    def get_node_label_list(self, nlabel_base_path, start_idx, duration, sep='\t'):
        """(per snapshot an int64 [rows, 2] tensor (node index, label) in file order, number of distinct labels over the window).
        Files are visited in sorted() order and have a header row; node names are mapped to indices."""
        return self._label_list(nlabel_base_path, start_idx, duration, sep, 1)

    def get_edge_label_list(self, elabel_base_path, start_idx, duration, sep='\t'):
        """(per snapshot an int64 [rows, 3] tensor (from index, to index, label) in file order, number of distinct labels)."""
        return self._label_list(elabel_base_path, start_idx, duration, sep, 2)

    # --------------------------------------------------- thin plumbing kept for reference-shaped drivers
    def get_date_adj_list(self, origin_base_path, start_idx, duration, sep='\t', normalize=False, row_norm=False,
                          add_eye=False, data_type='tensor'):
        """Snapshot adjacency matrices (reference helper.py:27-47).  Core-based methods only use them to derive edge lists
        (train.py:60-62).  normalize=True is what the baselines take: D^-1/2 (A [+ I]) D^-1/2, or D^-1 (A [+ I]) with row_norm, as a
        float32 sparse COO tensor on the loader's device (entries in row-major order; `_indices()` is the edge list) or, for
        data_type='matrix', as scipy COO.  The scaling runs on the GPU (ops.gcn_normalize) instead of the reference's np.vectorize call
        per node, so it needs has_cuda.  Two differences from the reference's float64 scipy arithmetic: the weights are cast to fp32
        before the upload (exact for the integer weights of the shipped datasets; other weights are normalised from their fp32
        rounding), then row sums, scales and products run in fp64 and are rounded to fp32 once; and data_type='matrix' returns those
        fp32 values in a float64 matrix, where the reference returns the unrounded float64 one."""
        assert data_type in ['tensor', 'matrix']
        files = sorted(os.listdir(origin_base_path))
        out = []
        for i in self._window(start_idx, duration):
            mat = get_sp_adj_mat(os.path.join(origin_base_path, files[i]), self.full_node_list, sep=sep)
            if add_eye:
                mat = (mat + sp.eye(mat.shape[0])).tocoo()
            if normalize:
                out.append(self._normalized(mat, row_norm, data_type))
                continue
            out.append(_coo_tensor(mat, self.device) if data_type == 'tensor' else mat)
        return out

    def _normalized(self, mat, row_norm, data_type):
        if not self.has_cuda:
            raise ops._lib.CtgcnHipError("the normalised adjacency is scaled by a HIP kernel: construct DataLoader(has_cuda=True); "
                                         "there is no CPU fallback")
        csr = sp.csr_matrix(mat)
        csr.sort_indices()
        if csr.nnz >= 2 ** 31:
            raise ValueError("more than 2^31-1 stored entries")
        row_ptr = torch.from_numpy(csr.indptr.astype(np.int32)).to(self.device)
        col = torch.from_numpy(csr.indices.astype(np.int32)).to(self.device)
        val = ops.gcn_normalize(row_ptr, col, torch.from_numpy(csr.data.astype(np.float32)).to(self.device), row_norm)
        coo = csr.tocoo()
        if data_type == 'matrix':
            return sp.coo_matrix((val.cpu().numpy().astype(np.float64), (coo.row, coo.col)), shape=csr.shape)
        idx = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64)).to(self.device)
        return torch.sparse_coo_tensor(idx, val, torch.Size(csr.shape))

    def get_degree_feature_list(self, origin_base_path, start_idx, duration, sep='\t', init_type='gaussian', std=1e-4):
        """Degree-based node features for the structural models CGCN-S / CTGCN-S (reference helper.py:109-158, called at
        train.py:72-74).  Returns (x_list, input_dim) with the reference's shapes, dtypes and layouts:

          degree   = int(weighted degree) of the snapshot's simple undirected graph (adj.sum(axis=1).astype(int), :121);
          D        = 1 + the largest degree over the WHOLE window (:122, :127-...);
          gaussian   dense float32 [N, D], row i ~ Normal(degree_i, std)                                   (:128-135)
          adj        sparse COO float32 [N, N] = the snapshot adjacency                                    (:136-139)
          combine    sparse COO float32 [N, D + N] = [gaussian | adj]                                      (:140-148)
          one-hot    sparse COO float32 [N, D], a single 1 in column degree_i                              (:149-156)

        Randomness: the reference draws from numpy's global RandomState row by row.  Without CUDA this loader draws the
        same stream in one vectorised call (same values bit for bit under np.random.seed).  With has_cuda the normals are
        generated on the GPU (torch Generator seeded from numpy's global state, so np.random.seed still makes a run
        reproducible): at config-3 scale the reference's host loop is 60 730 x 27 numpy calls and a 6.6 GB upload."""
        assert init_type in ['gaussian', 'adj', 'combine', 'one-hot']
        files = sorted(os.listdir(origin_base_path))
        adjs, degrees, max_degree = [], [], 0
        for i in self._window(start_idx, duration):
            adj = get_sp_adj_mat(os.path.join(origin_base_path, files[i]), self.full_node_list, sep=sep)
            deg = np.asarray(adj.sum(axis=1)).reshape(-1).astype(int)       # truncation toward zero, as astype(np.int)
            max_degree = max(max_degree, int(deg.max(initial=0)))
            adjs.append(adj)
            degrees.append(deg)
        x_list, input_dim = [], 0
        width = max_degree + 1
        for adj, deg in zip(adjs, degrees):
            if init_type == 'gaussian':
                # dense features built once and fed to every forward (train.py:72-76): the first Linear may keep their operand planes
                x_list.append(ops.mark_static(self._gaussian_degree_features(deg, std, width)))
                input_dim = width
            elif init_type == 'adj':
                x_list.append(_coo_tensor(adj, self.device))
                input_dim = self.node_num
            elif init_type == 'combine':
                # sp.coo_matrix(dense) keeps the non-zero entries in row-major order (exact zeros, probability ~0, dropped)
                gauss = np.random.normal(deg.reshape(-1, 1), std, (len(deg), width))
                feat = sp.hstack((sp.coo_matrix(gauss), adj)).astype(np.float32)
                x_list.append(_coo_tensor(feat, self.device))
                input_dim = feat.shape[1]
            else:
                idx = torch.from_numpy(np.vstack((np.arange(len(deg)), deg)).astype(np.int64))
                x_list.append(torch.sparse_coo_tensor(idx, torch.ones(len(deg), dtype=torch.float32),
                                                      torch.Size((len(deg), width))).to(self.device))
                input_dim = width
        return x_list, input_dim

    def _gaussian_degree_features(self, deg, std, width):
        if not self.has_cuda:
            return torch.from_numpy(np.random.normal(deg.reshape(-1, 1), std, (len(deg), width)).astype(np.float32))
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(np.random.randint(0, 2 ** 31 - 1)))
        x = torch.randn(len(deg), width, generator=gen, device=self.device, dtype=torch.float32)
        loc = torch.from_numpy(deg.astype(np.float32)).to(self.device)
        return x.mul_(float(std)).add_(loc.unsqueeze(1))

    def get_feature_list(self, feature_base_path, start_idx, duration, sep='\t', shuffle=False):
        """One-hot (sparse identity) node features when no feature files exist, else one dense float32 [rows, F] tensor per
        snapshot read from `<feature_base_path>/<sorted file i>` (header line, numeric columns), zero-padded on the right to
        the widest file of the window (reference helper.py:161-192)."""
        x_list = []
        if feature_base_path is None:
            for _ in self._window(start_idx, duration):
                cols = np.random.permutation(self.node_num) if shuffle else np.arange(self.node_num)
                mat = sp.coo_matrix((np.ones(self.node_num), (np.arange(self.node_num), cols)), shape=(self.node_num,) * 2)
                x_list.append(_coo_tensor(mat, self.device))
            return x_list, self.node_num
        import pandas as pd
        files = sorted(os.listdir(feature_base_path))
        arrays, width = [], 0
        for i in self._window(start_idx, duration):
            arr = pd.read_csv(os.path.join(feature_base_path, files[i]), sep=sep, header=0).values
            width = max(width, arr.shape[1])
            arrays.append(arr)
        for arr in arrays:
            full = np.zeros((arr.shape[0], width), dtype=np.float32)
            full[:, : arr.shape[1]] = arr
            x_list.append(ops.mark_static(torch.from_numpy(full).to(self.device)))
        return x_list, width


def _coo_tensor(mat, device):
    mat = mat.tocoo()
    idx = torch.from_numpy(np.vstack((mat.row, mat.col)).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(mat.data).float(), torch.Size(mat.shape)).to(device)


def core_adj_from_scipy(csr, max_core, device):
    """Upload a symmetric zero-diagonal scipy CSR and run the device builder (CoreAdj.from_graph)."""
    csr = sp.csr_matrix(csr)
    csr.sort_indices()
    if csr.nnz >= 2 ** 31:
        raise ValueError("more than 2^31-1 stored entries")
    row_ptr = torch.from_numpy(csr.indptr.astype(np.int32)).to(device)
    col = torch.from_numpy(csr.indices.astype(np.int32)).to(device)
    val = torch.from_numpy(csr.data.astype(np.float32)).to(device)
    return CoreAdj.from_graph(row_ptr, col, val, max_core=max_core)


def core_adj_from_edge_rows(src, dst, w, n, max_core, device):
    """Edge rows (numpy, file order) -> CoreAdj with every stage on the GPU: de-dup / symmetrise / CSR
    (ctgcn_edges_to_csr), k-core peel, level tags, slot reorder."""
    from . import ops
    s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).to(device)
    d = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int32)).to(device)
    ww = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(device)
    row_ptr, col, val = ops.edges_to_csr(s, d, ww, n)
    return CoreAdj.from_graph(row_ptr, col, val, max_core=max_core)
