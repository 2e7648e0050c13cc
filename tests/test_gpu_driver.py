"""The config-driven driver end to end on the bundled UCI snapshots (n = 1899, 7 months), through `ctgcn_amd.main.main`: the
preprocessing task once, then the embedding task of all 21 methods from the reference's UCI config, the loaders against what the
reference's get_input_data returned (golden/driver_uci.json), the driver against the hand-wired sequence, seeded reproducibility, the
supervised learning types, DynGEM's warm start, the time file and one evaluation task.

A case overrides base_path, epoch (2), seed and the range of its method's section; widths stay as configured.  Further keys are set only
where a case cannot be stated without them: another output folder for a second run, learning_type / duration / labels / the classifier
keys of the supervised cases (the UCI sections are unsupervised), record_time and load_model where they are the subject, and PGNN's
learning_type: its section says 'S-link', which the reference's own get_loss refuses, so the case runs it as 'S-link-st'."""
import copy
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

GNN = ['GCN', 'TgGCN', 'GAT', 'TgGAT', 'SAGE', 'TgSAGE', 'GIN', 'TgGIN', 'PGNN', 'CGCN-C', 'CGCN-S', 'GCRN', 'EvolveGCN', 'VGRNN', 'CTGCN-C',
       'CTGCN-S']
DYN = ['DynGEM', 'DynAE', 'DynRNN', 'DynAERNN']
ALL = DYN + ['TIMERS'] + GNN
N, T, SEED = 1899, 7, 7
DROP = object()         # an override that takes the key out of the section


class Dataset(object):
    def __init__(self, base, names, files, config):
        self.base, self.names, self.files, self.config = base, names, files, config
        self.runs = {}

    def path(self, *parts):
        return os.path.join(self.base, *parts)

    def write_config(self, config, name="config.json"):
        path = self.path(name)
        with open(path, "w") as fp:
            json.dump(config, fp)
        return path

    def section(self, method, **override):
        """the method's embedding section with the overrides every case makes, then the case's own"""
        args = dict(self.config["embedding"][method], base_path=self.base)
        if method != 'TIMERS':
            args.update(epoch=2, seed=SEED)
            if args["duration"] == 1:
                args["start_idx"] = -3
            elif method in DYN:
                args["start_idx"] = -2
        if method == 'PGNN':
            args["learning_type"] = 'S-link-st'
        args.update(override)
        return {k: v for k, v in args.items() if v is not DROP}

    def embed(self, method, tag="", **override):
        """run the embedding task through main(); returns {file name: bytes} of the embedding folder"""
        from ctgcn_amd.main import main
        args = self.section(method, **override)
        if tag:
            args["embed_folder"] = args["embed_folder"] + "_" + tag
        config = copy.deepcopy(self.config)
        config["embedding"][method] = args
        main(["prog", "--config", self.write_config(config, "config_%s_%s.json" % (method, tag)), "--task", "embedding", "--method", method])
        return read_folder(self.path(args["embed_folder"])), args

    def embed_once(self, method):
        """the seeded base run of a method, shared by the cases that only read it"""
        if method not in self.runs:
            self.runs[method] = self.embed(method)
        return self.runs[method]


def read_folder(path):
    out = {}
    for name in sorted(os.listdir(path)):
        with open(os.path.join(path, name), "rb") as fp:
            out[name] = fp.read()
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from ctgcn_amd.main import main
    base = str(tmp_path_factory.mktemp("uci"))
    snaps = load_golden("uci_snapshots.npz")
    names = [str(x) for x in snaps["node_names"]]
    files = [str(f) for f in snaps["files"]]
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    with open(os.path.join(base, "nodes_set", "nodes.csv"), "w") as fp:
        fp.write("\n".join(names) + "\n")
    for t, f in enumerate(files):
        with open(os.path.join(base, "1.format", f), "w") as fp:
            fp.write("from_id\tto_id\tweight\n")
            for s, d, w in zip(snaps["t%d_src" % t], snaps["t%d_dst" % t], snaps["t%d_w" % t]):
                fp.write("%s\t%s\t%d\n" % (names[s], names[d], int(w)))
    with open(os.path.join(GOLDEN, "uci_config.json")) as fp:
        config = json.load(fp)
    for task, section in config.items():
        for sub in (section.values() if task in ("embedding", "preprocessing") else [section]):
            sub["base_path"] = base
    config["preprocessing"]["CTGCN-C"].update(walk_time=10, seed=SEED)
    ds = Dataset(base, names, files, config)
    main(["prog", "--config", ds.write_config(config), "--task", "preprocessing", "--method", "CTGCN-C"])
    for folder in ("CTGCN/ctgcn_cores", "CTGCN/ctgcn_walk_pairs", "CTGCN/ctgcn_node_freq"):
        assert len(os.listdir(ds.path(folder))) == T, folder
    return ds


def expected_files(data, args, method):
    from ctgcn_amd.train import resolve_range
    if method == 'TIMERS':
        return list(data.files)
    start, end = resolve_range(T, args["start_idx"], args["end_idx"])
    return [f.split('.')[0] + '.csv' for f in data.files[start:end]]


# ------------------------------------------------------------------------------------------------ the embedding task, all 21 methods
@pytest.mark.parametrize("method", ALL)
def test_embedding_task_writes_every_snapshot_of_the_range(method, data):
    from ctgcn_amd.baseline import anchor_set_count
    files, args = data.embed_once(method)
    assert sorted(files) == expected_files(data, args, method)
    width = anchor_set_count(N) if method == 'PGNN' else args["embed_dim"]
    for name in files:
        df = pd.read_csv(data.path(args["embed_folder"], name), sep="\t", index_col=0)
        assert df.shape == (N, width), (name, df.shape)
        assert [str(x) for x in df.index] == data.names
        assert np.isfinite(df.values).all(), name
    if method != 'TIMERS':
        assert os.path.getsize(data.path(args["model_folder"], args["model_file"])) > 0


# ------------------------------------------------------------------------------------------------ loaders against the reference
@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "driver_uci.json")) as fp:
        return json.load(fp)


def _stats(t):
    return [int(t._values().numel()), float(t._values().double().sum())]


def _check_stats(got, want, what):
    assert got[0] == want[0], (what, got, want)
    # the loader rounds every value to fp32 once (2^-24 relative each), the reference sums float64 values
    assert abs(got[1] - want[1]) <= 1e-6 * abs(want[1]), (what, got, want)


@pytest.mark.parametrize("method", GNN)
def test_get_input_data_matches_what_the_reference_returned(method, data, recorded):
    from ctgcn_amd import train
    want = recorded["methods"][method]
    idx, time_length = recorded["window"]
    args = dict(data.section(method), has_cuda=True)
    np.random.seed(1)
    loader = train.get_data_loader(args)
    assert loader.max_time_num == recorded["max_time_num"] and args["node_num"] == N
    input_dim, adj_list, x_list, edge_list, node_dist_list = train.get_input_data(method, idx, time_length, loader, args)
    assert input_dim == want["input_dim"]
    assert (adj_list is None) == want["adj_none"]
    assert [list(e.shape) for e in edge_list] == want["edge_shapes"] and all(e.is_cuda and e.dtype == torch.int64 for e in edge_list)
    if adj_list is not None:
        assert len(adj_list) == len(want["adj"]) == time_length
        for t, (adj, ref) in enumerate(zip(adj_list, want["adj"])):
            if isinstance(ref[0], list):                                # core-based: one pair per k-core matrix
                mats = adj.to_scipy_list()
                assert len(adj) == len(mats) == len(ref), (t, len(mats), len(ref))
                for j, (m, r) in enumerate(zip(mats, ref)):
                    _check_stats([int(m.nnz), float(m.data.astype(np.float64).sum())], r, (method, t, j))
            else:
                assert tuple(adj.shape) == (N, N)
                _check_stats(_stats(adj), ref, (method, t))
    if isinstance(x_list, torch.Tensor):
        kind, shape = ("stacked-sparse" if x_list.is_sparse else "stacked-dense"), list(x_list.shape)
    else:
        kinds = {("sparse" if x.is_sparse else "dense") for x in x_list}
        assert len(kinds) == 1
        kind, shape = kinds.pop(), [list(x.shape) for x in x_list]
    assert (kind, shape) == (want["x_kind"], want["x_shape"])
    if method == 'PGNN':
        assert len(node_dist_list) == len(want["dist_shapes"]) and all(d.num_nodes == N and d.cutoff == -1 for d in node_dist_list)
    else:
        assert node_dist_list is None and "dist_shapes" not in want


# ------------------------------------------------------------------------------------------------ the driver against the hand-wired run
def _hand_wired(method, data, args, folder):
    """loader -> model -> loss -> trainer per window, written out stage by stage with the method's rules spelled out"""
    import random
    import ctgcn_amd
    windows = {'GCN': [(4, 1), (5, 1), (6, 1)], 'CTGCN-C': [(0, 7)], 'EvolveGCN': [(0, 7)]}[method]
    origin = data.path("1.format")
    for idx, tl in windows:
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        random.seed(SEED)
        dl = ctgcn_amd.DataLoader(data.names, T, has_cuda=True)
        if method == 'GCN':
            adj = dl.get_date_adj_list(origin, idx, tl, sep="\t", normalize=True, row_norm=True, add_eye=True, data_type='tensor')
            edges = [a._indices() for a in adj]
            x, dim = dl.get_feature_list(None, idx, tl, shuffle=False)
            model = ctgcn_amd.GCN(dim, 500, 128, dropout=0.5, bias=True)
        elif method == 'EvolveGCN':
            adj = dl.get_date_adj_list(origin, idx, tl, sep="\t", normalize=True, row_norm=False, add_eye=True, data_type='tensor')
            edges = [a._indices() for a in adj]
            x, dim = dl.get_degree_feature_list(origin, idx, tl, sep="\t", init_type='gaussian', std=1e-4)
            model = ctgcn_amd.EvolveGCN(dim, 128, 128, egcn_type='EGCNH')
        else:
            core = dl.get_core_adj_list(data.path("CTGCN/ctgcn_cores"), idx, tl, max_core=-1)
            raw = dl.get_date_adj_list(origin, idx, tl, sep="\t", normalize=False, row_norm=False, add_eye=False, data_type='tensor')
            edges = [a._indices() for a in raw]
            adj = core
            x, dim = dl.get_feature_list(None, idx, tl, shuffle=False)
            model = ctgcn_amd.CTGCN(dim, 500, 128, trans_num=1, diffusion_num=2, duration=tl, bias=True, rnn_type='GRU', model_type='C',
                                    trans_activate_type='L')
        pairs = dl.get_node_pair_list(data.path("CTGCN/ctgcn_walk_pairs"), idx, tl)
        freqs = dl.get_node_freq_list(data.path("CTGCN/ctgcn_node_freq"), idx, tl)
        loss = ctgcn_amd.NegativeSamplingLoss(pairs, freqs, neg_num=20, Q=20, seed=SEED)
        trainer = ctgcn_amd.UnsupervisedEmbedding(data.base, "1.format", folder, data.names, model, loss, model_folder="hand/model", has_cuda=True)
        trainer.learn_embedding(adj, x, edges, None, epoch=2, batch_size=2048, lr=1e-3, start_idx=idx, weight_decay=5e-4,
                                model_file=args["model_file"], load_model=False, shuffle=True, export=True)
    return read_folder(data.path(folder))


@pytest.mark.parametrize("method", ['CTGCN-C', 'GCN', 'EvolveGCN'])
def test_the_driver_writes_the_bytes_of_the_hand_wired_sequence(method, data):
    files, args = data.embed_once(method)
    hand = _hand_wired(method, data, args, "hand/" + method)
    assert sorted(hand) == sorted(files) and len(files) > 0
    for name in files:
        assert hand[name] == files[name], name


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("method", ['CTGCN-C', 'CTGCN-S', 'GCN', 'EvolveGCN', 'VGRNN'])
def test_two_seeded_runs_write_identical_bytes(method, data):
    first, _ = data.embed_once(method)
    second, _ = data.embed(method, tag="again")
    assert sorted(first) == sorted(second) and len(first) > 0
    for name in first:
        assert first[name] == second[name], name


def test_two_unseeded_runs_differ(data):
    outs = [data.embed('GCN', tag=tag, seed=DROP)[0] for tag in ("free1", "free2")]
    assert sorted(outs[0]) == sorted(outs[1]) and any(outs[0][k] != outs[1][k] for k in outs[0])


# ------------------------------------------------------------------------------------------------ supervised learning types
@pytest.mark.parametrize("method", ['CTGCN-C', 'GCN'])
@pytest.mark.parametrize("learning_type", ['S-link-st', 'S-link-dy'])
def test_link_supervision_exports_the_windows_of_its_schedule(method, learning_type, data):
    from ctgcn_amd.train import window_schedule
    files, args = data.embed(method, tag=learning_type, learning_type=learning_type, duration=3, start_idx=0, end_idx=-1, record_time=True)
    schedule = window_schedule(T, 0, -1, 3, learning_type)
    if learning_type == 'S-link-dy':
        assert schedule == [(0, 3), (2, 3), (4, 2)]
        covered = sorted({idx + i for idx, tl in schedule for i in range(tl - 1)})      # a window's last snapshot is a target only
    else:
        assert schedule == [(0, 3), (3, 3), (6, 1)]
        covered = list(range(T))
    assert sorted(files) == [data.files[t].split('.')[0] + '.csv' for t in covered]
    for name in files:
        df = pd.read_csv(data.path(args["embed_folder"], name), sep="\t", index_col=0)
        assert df.shape == (N, 128) and np.isfinite(df.values).all()
    assert len(pd.read_csv(data.path(method + "_time.csv"))) == len(schedule)


def test_node_supervision_on_cgcn_c_with_labels_the_test_writes(data):
    os.makedirs(data.path("nlabels"), exist_ok=True)
    rng = np.random.default_rng(3)
    for f in data.files:
        with open(data.path("nlabels", f), "w") as fp:
            fp.write("node\tlabel\n")
            for i in rng.permutation(N)[:1200]:
                fp.write("%s\t%d\n" % (data.names[i], i % 3))
    files, args = data.embed('CGCN-C', tag="node", learning_type='S-node', nlabel_folder="nlabels", cls_hid_dim=64, cls_layer_num=1,
                             cls_bias=True, cls_activate_type='N', cls_file="cgcn-c_cls")
    assert sorted(files) == expected_files(data, args, 'CGCN-C') and len(files) == 3
    for name in files:
        df = pd.read_csv(data.path(args["embed_folder"], name), sep="\t", index_col=0)
        assert df.shape == (N, 128) and np.isfinite(df.values).all()


# ------------------------------------------------------------------------------------------------ DynGEM's warm start
@pytest.mark.parametrize("load_model", [True, False])
def test_dyngem_windows_start_from_the_previous_checkpoint_only_with_load_model(load_model, data, monkeypatch):
    from ctgcn_amd.baseline import DynamicEmbedding
    seen = []
    prepare = DynamicEmbedding.prepare

    def recording(self, load, model_file, **kwargs):
        path = os.path.join(self.model_base_path, model_file)
        on_disk = torch.load(path, map_location="cpu") if seen and os.path.exists(path) else None
        out = prepare(self, load, model_file, **kwargs)
        seen.append((on_disk, {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}))
        return out

    monkeypatch.setattr(DynamicEmbedding, "prepare", recording)
    tag = "warm" if load_model else "cold"
    files, args = data.embed('DynGEM', tag=tag, load_model=load_model, model_file="dyngem_" + tag, start_idx=-2)
    assert len(seen) == 2 and len(files) == 2
    saved_by_first, start_of_second = seen[1]
    assert saved_by_first is not None and sorted(saved_by_first) == sorted(start_of_second)
    same = all(torch.equal(saved_by_first[k], start_of_second[k]) for k in saved_by_first)
    moved = any(not torch.equal(seen[0][1][k], saved_by_first[k]) for k in saved_by_first)
    assert moved                                    # the first window trained: its checkpoint is not its initial state
    assert same == load_model


# ------------------------------------------------------------------------------------------------ record_time
@pytest.mark.parametrize("method,windows", [('CGCN-C', 3), ('DynAE', 2)])
def test_record_time_writes_one_row_per_window(method, windows, data):
    data.embed(method, tag="timed", record_time=True)
    df = pd.read_csv(data.path(method + "_time.csv"))
    assert list(df.columns) == ["time"] and len(df) == windows and (df["time"] > 0).all()


# ------------------------------------------------------------------------------------------------ an evaluation task
def test_link_pred_task_over_the_exported_gcn_embeddings(data):
    from ctgcn_amd.main import main
    data.embed_once('GCN')                                              # snapshots 4, 5, 6: the task predicts 5 from 4 and 6 from 5
    config = copy.deepcopy(data.config)
    config["link_pred"].update(generate=True, method_list=['GCN'], seed=SEED)
    main(["prog", "--config", data.write_config(config, "config_lp.json"), "--task", "link_pred"])
    for f in data.files:
        for part in ("train", "val", "test"):
            assert os.path.getsize(data.path("lp_data_0", "%s_%s.csv" % (f.split('.')[0], part))) > 0
    df = pd.read_csv(data.path("lp_res_0", "GCN_auc_record.csv"))
    assert list(df.columns) == ["date", "Avg", "Had", "L1", "L2"] and list(df["date"]) == ["2004-09", "2004-10"]
    assert ((df.iloc[:, 1:].values > 0) & (df.iloc[:, 1:].values <= 1)).all()
