"""Link-prediction evaluation with the reference's interface and file contract (evaluation/link_prediction.py), on the GPU.

DataGenerator / LinkPredictor / aggregate_results / link_prediction(args) keep the reference's constructor and method signatures,
config keys and file formats: lp-data written by either implementation is read by the other.  What runs differently:
  - negatives are drawn by one GPU launch per snapshot (ctgcn_lp_neg_sample, counter RNG keyed on (seed, slot)) instead of a
    Python loop over a dict; the split counts, slicing order and positives-then-negatives layout are the reference's;
  - the 4 measures x |C| balanced logistic regressions of a snapshot are fitted together by the GPU Newton solver of _logreg.py to
    tol (default 1e-6 on sklearn's scaled gradient, where the reference's lbfgs stops at 1e-4), with no [E, d] feature matrices;
  - AUCs are roc_auc_score of expit(z) in float64.
`worker` is accepted and ignored.  evaluate() is the in-memory entry point; evaluate_window() runs it over a window of embeddings
with splits drawn by the GPU sampler.
"""
import os
import time
import zlib
from functools import partial

import numpy as np
import pandas as pd
import torch

from .. import _lib
from .._lib import check, ptr
from . import _common, _logreg
from ._common import aggregate_stats, method_snapshots, read_embedding, read_nodes, select_C
from ._logreg import EdgeSet, require_cuda, roc_auc

ALL_MEASURES = ("Avg", "Had", "L1", "L2", "sigmoid")
MAX_ATTEMPTS = 1 << 20        # draws per negative slot before the sampler gives up (expected: 1 / fraction of valid pairs)


_device = partial(_common.device, task="link-prediction")


def split_counts(edge_num, train_ratio, val_ratio, test_ratio):
    """(train_num, val_num, test_num) of a snapshot with edge_num directed rows, as the reference computes them."""
    test_num = int(np.floor(edge_num * test_ratio))
    val_num = int(np.floor(edge_num * val_ratio))
    train_num = int(np.floor((edge_num - test_num - val_num) * train_ratio))
    return train_num, val_num, test_num


def membership_keys(pos, n_nodes):
    """Sorted unique int64 keys u * n_nodes + v of the rows of pos ([E, 2], both directions already present)."""
    return torch.unique(pos[:, 0] * n_nodes + pos[:, 1])


def valid_pair_count(keys, n_nodes):
    """Ordered pairs (u, v), u != v, with neither direction in the (symmetric) key set."""
    off_diag = int(((keys // n_nodes) != (keys % n_nodes)).sum())
    return n_nodes * (n_nodes - 1) - off_diag


def sample_negatives(keys, n_nodes, count, seed, device):
    """count negative edges [count, 2] (int64) of the graph whose membership keys are `keys`; output depends on (seed, slot) only."""
    keys = keys.to(device=device, dtype=torch.int64).contiguous()
    if n_nodes < 2 or valid_pair_count(keys, n_nodes) <= 0:
        raise ValueError("no ordered pair (u, v) with u != v is a non-edge in either direction: no negative edge can be drawn")
    out = torch.empty(2, max(count, 1), dtype=torch.int64, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    check(_lib.load().ctgcn_lp_neg_sample(count, n_nodes, ptr(keys), keys.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, MAX_ATTEMPTS,
                                          ptr(out[0]), ptr(out[1]), ptr(flag), torch.cuda.current_stream(device).cuda_stream),
          "ctgcn_lp_neg_sample")
    return out[:, :count].t()


def make_splits(pos, n_nodes, train_ratio, val_ratio, test_ratio, seed, device=None):
    """The reference's generate_edge_sample on a GPU edge list pos ([lines, 2] int64, one row per file line): both directions of
    every row with label 1, shuffled, sliced val / test / train, each split followed by as many negatives (label 0).  Returns
    (train, val, test) as [n, 3] int64 tensors."""
    require_cuda(pos, "edge list")
    assert train_ratio + test_ratio + val_ratio <= 1.0
    device = pos.device
    pos = pos.to(torch.int64)
    both = torch.stack([pos, pos.flip(1)], 1).reshape(-1, 2)
    edge_num = both.shape[0]
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    both = both[torch.randperm(edge_num, generator=gen, device=device)]
    train_num, val_num, test_num = split_counts(edge_num, train_ratio, val_ratio, test_ratio)
    neg = sample_negatives(membership_keys(both, n_nodes), n_nodes, train_num + test_num + val_num,
                           (int(seed) * 0x9E3779B97F4A7C15 + 1) & 0xFFFFFFFFFFFFFFFF, device)
    return assemble_splits(both, neg, train_ratio, val_ratio, test_ratio)


def assemble_splits(shuffled, neg, train_ratio, val_ratio, test_ratio):
    """shuffled: [E, 2] positive rows in shuffled order; neg: [train_num + test_num + val_num, 2] negatives (train's, then test's, then
    val's).  Positives are sliced val, test, train as the reference does; each split is its positives (label 1) then its negatives
    (label 0).  Returns (train, val, test) [n, 3] int64."""
    train_num, val_num, test_num = split_counts(shuffled.shape[0], train_ratio, val_ratio, test_ratio)
    val_pos = shuffled[:val_num]
    test_pos = shuffled[val_num:val_num + test_num]
    train_pos = shuffled[val_num + test_num:val_num + test_num + train_num]
    negs = torch.split(neg, [train_num, test_num, val_num])

    def stack(p, q):
        ones = torch.ones(p.shape[0], 1, dtype=torch.int64, device=p.device)
        zeros = torch.zeros(q.shape[0], 1, dtype=torch.int64, device=q.device)
        return torch.cat([torch.cat([p, ones], 1), torch.cat([q, zeros], 1)], 0)

    return stack(train_pos, negs[0]), stack(val_pos, negs[2]), stack(test_pos, negs[1])


def write_split(path, edges, sep):
    """One lp-data file: header from_id, to_id, label; sep = the config's file_sep."""
    pd.DataFrame(edges.cpu().numpy(), columns=['from_id', 'to_id', 'label']).to_csv(path, sep=sep, index=False)


def _sigmoid_score(E, es):
    out = torch.empty(es.n, dtype=torch.float64, device=E.device)
    step = 1 << 20
    for s in range(0, es.n, step):
        a = E[es.src[s:s + step]].to(torch.float64)
        b = E[es.dst[s:s + step]].to(torch.float64)
        out[s:s + step] = torch.sigmoid((a * b).sum(1))
    return out


def evaluate(embedding_prev, train, val, test, C_list, measure_list, max_iter=100, tol=1e-6, hess_max=1 << 18):
    """In-memory link prediction of one snapshot.  embedding_prev: float32 CUDA [N, d]; train / val / test: [n, 3] int64 CUDA
    (from_id, to_id, label).  For every measure other than 'sigmoid' and every C a balanced logistic regression is fitted on train;
    the C with the best validation AUC (the last of ties) is kept and its test AUC reported.  Returns a dict:
      auc[measure]      test AUC (for 'sigmoid': AUC of σ(a·b), no model)
      C[measure]        the chosen C
      val_auc[measure]  validation AUC per C
      report            the solver's FitReport of every fitted model
    max_iter caps Newton iterations."""
    require_cuda(embedding_prev, "embedding_prev")
    for m in measure_list:
        if m not in ALL_MEASURES:
            raise ValueError("unknown measure %r" % (m,))
    E = embedding_prev.to(torch.float32).contiguous()
    n_nodes = E.shape[0]
    tr, va, te = (EdgeSet(x, n_nodes) for x in (train, val, test))
    lr_measures = [m for m in measure_list if m != 'sigmoid']
    models = [(m, C) for m in lr_measures for C in C_list]
    res = {"auc": {}, "C": {}, "val_auc": {}, "report": []}
    if models:
        theta, res["report"] = _logreg.fit(E, tr, [m for m, _ in models], [C for _, C in models], tol=tol, max_iter=max_iter,
                                           hess_max=hess_max)
        z_val = _logreg.scores_all(E, va, [m for m, _ in models], theta)
        z_test = _logreg.scores_all(E, te, [m for m, _ in models], theta)
        for mi, measure in enumerate(lr_measures):
            rows = range(mi * len(C_list), (mi + 1) * len(C_list))
            aucs = [roc_auc(va.label, torch.sigmoid(z_val[r].to(torch.float64))) for r in rows]
            idx = select_C(aucs)
            res["val_auc"][measure] = aucs
            res["C"][measure] = C_list[idx]
            res["auc"][measure] = roc_auc(te.label, torch.sigmoid(z_test[rows[idx]].to(torch.float64)))
    if 'sigmoid' in measure_list:
        res["auc"]['sigmoid'] = roc_auc(te.label, _sigmoid_score(E, te))
    return res


def evaluate_window(embeddings, snapshot_edges, C_list, measure_list, train_ratio=0.5, val_ratio=0.3, test_ratio=0.2, seed=0,
                    max_iter=100, tol=1e-6):
    """Link prediction over a window: snapshot i >= 1 is predicted from embeddings[i-1], with splits of snapshot_edges[i] ([lines, 2]
    CUDA int64, one row per undirected edge) drawn by make_splits under seed + i.  embeddings: CUDA [N, T, d] or a list of [N, d].
    Returns one evaluate() result per predicted snapshot."""
    if isinstance(embeddings, torch.Tensor) and embeddings.dim() == 3:
        embeddings = [embeddings[:, t] for t in range(embeddings.shape[1])]
    out = []
    for i in range(1, len(snapshot_edges)):
        E = embeddings[i - 1]
        train, val, test = make_splits(snapshot_edges[i], E.shape[0], train_ratio, val_ratio, test_ratio, seed + i)
        out.append(evaluate(E, train, val, test, C_list, measure_list, max_iter=max_iter, tol=tol))
    return out


class DataGenerator(object):
    """Reference DataGenerator: writes <date>_{train,val,test}.csv per snapshot file.  seed: 64-bit seed of the GPU draws; None draws
    one from np.random, so np.random.seed(...) reproduces a run."""

    def __init__(self, base_path, input_folder, output_folder, node_file, file_sep='\t', train_ratio=0.5, val_ratio=0.2, test_ratio=0.3,
                 seed=None, device=None):
        self.base_path = base_path
        self.input_base_path = os.path.join(base_path, input_folder)
        self.output_base_path = os.path.join(base_path, output_folder)
        self.file_sep = file_sep
        self.full_node_list = read_nodes(os.path.join(base_path, node_file))
        self.node_num = len(self.full_node_list)
        self.node2idx_dict = dict(zip(self.full_node_list, np.arange(self.node_num)))
        assert train_ratio + test_ratio + val_ratio <= 1.0
        self.train_ratio, self.val_ratio, self.test_ratio = train_ratio, val_ratio, test_ratio
        self.seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if seed is None else int(seed)
        self.device = device
        os.makedirs(self.input_base_path, exist_ok=True)
        os.makedirs(self.output_base_path, exist_ok=True)

    def read_edges(self, file, sep='\t'):
        """[lines, 2] int64 node indices of a snapshot edge file (header skipped, names mapped through nodes_set)."""
        df = pd.read_csv(os.path.join(self.input_base_path, file), sep=sep, header=0, dtype=str, keep_default_na=False, usecols=[0, 1])
        idx = pd.Index([str(n) for n in self.full_node_list]).get_indexer(pd.concat([df.iloc[:, 0], df.iloc[:, 1]]).str.strip())
        if (idx < 0).any():
            raise KeyError("edge endpoint not in the node file: %s" % file)
        return torch.from_numpy(idx.reshape(2, -1).T.astype(np.int64).copy())

    def generate_edge_sample(self, file, sep='\t'):
        date = file.split('.')[0]
        pos = self.read_edges(file, sep).to(_device(self.device))
        seed = self.seed ^ zlib.crc32(date.encode('utf-8'))
        train, val, test = make_splits(pos, self.node_num, self.train_ratio, self.val_ratio, self.test_ratio, seed)
        write_split(os.path.join(self.output_base_path, date + '_train.csv'), train, self.file_sep)
        write_split(os.path.join(self.output_base_path, date + '_test.csv'), test, self.file_sep)
        write_split(os.path.join(self.output_base_path, date + '_val.csv'), val, self.file_sep)

    def generate_edge_samples_all_time(self, sep='\t', worker=-1):
        for file_name in sorted(os.listdir(self.input_base_path)):
            self.generate_edge_sample(file_name, sep=sep)


class LinkPredictor(object):
    """Reference LinkPredictor: <method>_auc_record.csv (columns date + measures, sep ',') under output_folder.  tol: the solver's
    stopping tolerance on max |∇f|; max_iter caps Newton iterations at min(max_iter, 100)."""

    def __init__(self, base_path, origin_folder, embedding_folder, lp_edge_folder, output_folder, node_file, file_sep='\t', C_list=None,
                 measure_list=None, max_iter=5000, tol=1e-6, device=None):
        self.base_path = base_path
        self.origin_base_path = os.path.join(base_path, origin_folder)
        self.embedding_base_path = os.path.join(base_path, embedding_folder)
        self.lp_edge_base_path = os.path.join(base_path, lp_edge_folder)
        self.output_base_path = os.path.join(base_path, output_folder)
        self.file_sep = file_sep
        self.measure_list = measure_list
        self.full_node_list = read_nodes(os.path.join(base_path, node_file))
        self.C_list = C_list
        self.max_iter = max_iter
        self.tol = tol
        self.device = device
        self.reports = {}
        for p in (self.embedding_base_path, self.origin_base_path, self.output_base_path):
            os.makedirs(p, exist_ok=True)

    def _read_split(self, date, part, dev):
        arr = pd.read_csv(os.path.join(self.lp_edge_base_path, date + '_' + part + '.csv'), sep=self.file_sep).values
        return torch.from_numpy(arr.astype(np.int64)).to(dev)

    def link_prediction_all_time(self, method):
        dev = _device(self.device)

        def read_splits(date):
            return [self._read_split(date, p, dev) for p in ('train', 'val', 'test')]

        rows = []
        for date, _, pre_embedding_path, (train, val, test) in method_snapshots(self.origin_base_path, self.embedding_base_path, method,
                                                                               lag=1, first=read_splits):
            E = torch.from_numpy(read_embedding(pre_embedding_path, self.file_sep, self.full_node_list, np.float32)).to(dev)
            res = evaluate(E, train, val, test, self.C_list, self.measure_list, max_iter=min(self.max_iter, 100), tol=self.tol)
            self.reports[(method, date)] = res
            rows.append([date] + [res["auc"][m] for m in self.measure_list])
        df_output = pd.DataFrame(rows, columns=['date'] + list(self.measure_list))
        print(df_output)
        df_output.to_csv(os.path.join(self.output_base_path, method + '_auc_record.csv'), sep=',', index=False)

    def link_prediction_all_method(self, method_list=None, worker=-1):
        if method_list is None:
            method_list = os.listdir(self.embedding_base_path)
        for method in method_list:
            self.link_prediction_all_time(method)


def aggregate_results(base_path, lp_res_folder, start_idx, rep_num, method_list, measure_list):
    """Per method and measure: <method>_<measure>_record.csv under lp_res_folder with date, one AUC column per repetition
    (<measure>_<i>), then avg, max, min over the repetitions."""
    if rep_num <= 0:
        return
    reps = range(start_idx, start_idx + rep_num)
    out_dir = os.path.join(base_path, lp_res_folder)
    os.makedirs(out_dir, exist_ok=True)
    for method in method_list:
        tables = {}
        for i in reps:
            path = os.path.join(base_path, lp_res_folder + '_' + str(i), method + '_auc_record.csv')
            tables[i] = pd.read_csv(path, sep=',', header=0, names=['date'] + [m + '_' + str(i) for m in measure_list])
        for m in measure_list:
            cols = [m + '_' + str(i) for i in reps]
            df = pd.concat([tables[start_idx].loc[:, ['date', cols[0]]].copy()] + [tables[i].loc[:, [m + '_' + str(i)]] for i in reps[1:]],
                           axis=1)
            aggregate_stats(df, cols).to_csv(os.path.join(out_dir, method + '_' + m + '_record.csv'), sep=',', index=False)


def link_prediction(args):
    """The reference's link_pred driver: the same config keys ('worker' ignored; optional 'tol' and 'seed')."""
    base_path = args['base_path']
    start_idx, rep_num = args['start_idx'], args['rep_num']
    if args['do_lp']:
        for i in range(start_idx, start_idx + rep_num):
            seed = args.get('seed')
            data_generator = DataGenerator(base_path=base_path, input_folder=args['origin_folder'],
                                           output_folder=args['lp_edge_folder'] + '_' + str(i), node_file=args['node_file'],
                                           file_sep=args['file_sep'], train_ratio=args['train_ratio'], val_ratio=args['val_ratio'],
                                           test_ratio=args['test_ratio'], seed=None if seed is None else seed + i)
            if args['generate']:
                data_generator.generate_edge_samples_all_time(sep=args['file_sep'])
            link_predictor = LinkPredictor(base_path=base_path, origin_folder=args['origin_folder'], embedding_folder=args['embed_folder'],
                                           lp_edge_folder=args['lp_edge_folder'] + '_' + str(i),
                                           output_folder=args['lp_res_folder'] + '_' + str(i), node_file=args['node_file'],
                                           file_sep=args['file_sep'], C_list=args['c_list'], measure_list=args['measure_list'],
                                           max_iter=args['max_iter'], tol=args.get('tol', 1e-6))
            t1 = time.time()
            link_predictor.link_prediction_all_method(method_list=args['method_list'])
            print('link prediction cost time: ', time.time() - t1, ' seconds!')
    if args['aggregate']:
        aggregate_results(base_path, args['lp_res_folder'], start_idx, rep_num, args['method_list'], args['measure_list'])
