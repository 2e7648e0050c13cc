"""The config-driven driver without a GPU: method tables, window arithmetic, the per-method input rules against a recording stub
loader, model and loss construction from the reference's UCI config, the command line's dispatch, and the trainers' acceptance of
this package's own GCN.  Expected values recorded from the reference are in golden/driver_uci.json (make_golden_driver.py)."""
import copy
import json
import os

import pytest
import torch

from conftest import GOLDEN

GNN = ['GCN', 'TgGCN', 'GAT', 'TgGAT', 'SAGE', 'TgSAGE', 'GIN', 'TgGIN', 'PGNN', 'CGCN-C', 'CGCN-S', 'GCRN', 'EvolveGCN', 'VGRNN', 'CTGCN-C',
       'CTGCN-S']
NON_GNN = ['DynGEM', 'DynAE', 'DynRNN', 'DynAERNN', 'TIMERS']
NO_ADJ = {'TgGCN', 'TgGAT', 'TgSAGE', 'TgGIN', 'PGNN'}
CORE = ['CGCN-C', 'CGCN-S', 'CTGCN-C', 'CTGCN-S']


@pytest.fixture(scope="module")
def config():
    with open(os.path.join(GOLDEN, "uci_config.json")) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "driver_uci.json")) as fp:
        return json.load(fp)


# ------------------------------------------------------------------------------------------------ method tables
def test_method_tables_hold_the_reference_s_names_in_its_order(recorded):
    from ctgcn_amd import utils
    assert list(utils.get_static_gnn_methods()) == GNN[:11]
    assert list(utils.get_dynamic_gnn_methods()) == GNN[11:]
    assert list(utils.get_core_based_methods()) == CORE
    assert list(utils.get_supported_gnn_methods()) == GNN and len(utils.get_supported_gnn_methods()) == 16
    assert list(utils.get_supported_methods()) == NON_GNN + GNN and len(utils.get_supported_methods()) == 21
    assert 'GCN' in utils.get_supported_gnn_methods() and 'TIMERS' not in utils.get_supported_gnn_methods()
    assert 'TIMERS' in utils.get_supported_methods() and 'node2vec' not in utils.get_supported_methods()
    for name, want in recorded["method_tables"].items():
        assert list(getattr(utils, name)()) == want, name


# ------------------------------------------------------------------------------------------------ window arithmetic
def test_window_schedule_matches_the_stated_cases_and_the_reference_s_loop(recorded):
    from ctgcn_amd.train import window_schedule
    assert window_schedule(7, 0, -1, 3, 'U-neg') == [(0, 3), (3, 3), (6, 1)]
    assert window_schedule(7, 0, -1, 3, 'S-link-dy') == [(0, 3), (2, 3), (4, 2)]
    assert window_schedule(7, -3, -1, 1, 'U-neg') == [(4, 1), (5, 1), (6, 1)]
    assert len(recorded["schedules"]) >= 9
    for case in recorded["schedules"]:
        call = (case["max_time_num"], case["start_idx"], case["end_idx"], case["duration"], case["learning_type"])
        if case["raises"]:
            with pytest.raises(AssertionError):
                window_schedule(*call)
        else:
            assert window_schedule(*call) == [tuple(w) for w in case["windows"]], call
    with pytest.raises(AssertionError):
        window_schedule(7, 0, -1, 1, 'S-link-dy')


# ------------------------------------------------------------------------------------------------ get_input_data
class StubLoader(object):
    """records every loader call; returns small stand-ins of the right kinds"""

    def __init__(self, n=5):
        self.n, self.calls = n, []

    def _eye(self):
        i = torch.arange(self.n)
        return torch.sparse_coo_tensor(torch.stack([i, i]), torch.ones(self.n), (self.n, self.n))

    def get_core_adj_list(self, path, start_idx, duration, max_core=-1):
        self.calls.append(("core", path, start_idx, duration, max_core))
        return ["core%d" % t for t in range(duration)]

    def get_date_adj_list(self, path, start_idx, duration, sep='\t', normalize=False, row_norm=False, add_eye=False, data_type='tensor'):
        self.calls.append(("adj", path, start_idx, duration, sep, normalize, row_norm, add_eye, data_type))
        return [self._eye() for _ in range(duration)]

    def get_degree_feature_list(self, path, start_idx, duration, sep='\t', init_type='gaussian', std=1e-4):
        self.calls.append(("degree", path, start_idx, duration, sep, init_type, std))
        return [torch.zeros(self.n, 3) for _ in range(duration)], 3

    def get_feature_list(self, path, start_idx, duration, sep='\t', shuffle=False):
        self.calls.append(("feature", path, start_idx, duration, shuffle))
        return [self._eye() for _ in range(duration)], self.n


def _norm_triple(method):
    if method in ('GCN', 'GAT', 'GCRN'):
        return (True, True, True)
    if method == 'EvolveGCN':
        return (True, False, True)
    return (False, False, False)


@pytest.mark.parametrize("method", GNN)
def test_get_input_data_follows_the_per_method_rules(method, config, monkeypatch):
    from ctgcn_amd import train
    from ctgcn_amd.baseline import pgnn
    dist_calls = []
    monkeypatch.setattr(pgnn, "precompute_dist_data", lambda edges, n, approximate: dist_calls.append((len(edges), n, approximate)) or "dist")
    args = dict(config["embedding"][method], origin_base_path="/o", core_base_path="/c", nfeature_path=None, node_num=5)
    loader = StubLoader()
    input_dim, adj_list, x_list, edge_list, node_dist_list = train.get_input_data(method, 4, 3, loader, args)
    kinds = [c[0] for c in loader.calls]
    adj_call = [c for c in loader.calls if c[0] == "adj"]
    assert len(adj_call) == 1 and adj_call[0][1:5] == ("/o", 4, 3, "\t")
    assert adj_call[0][5:8] == _norm_triple(method) and adj_call[0][8] == 'tensor'
    assert train.adjacency_normalisation(method) == _norm_triple(method)
    assert len(edge_list) == 3 and all(tuple(e.shape) == (2, 5) for e in edge_list)
    if method in CORE:
        assert ("core", "/c", 4, 3, args["max_core"]) in loader.calls and adj_list == ["core0", "core1", "core2"]
    else:
        assert "core" not in kinds
        assert (adj_list is None) == (method in NO_ADJ)
    if method in ('EvolveGCN', 'CGCN-S', 'CTGCN-S'):
        assert ("degree", "/o", 4, 3, "\t", args["init_type"], args["std"]) in loader.calls and "feature" not in kinds and input_dim == 3
    else:
        assert ("feature", None, 4, 3, False) in loader.calls and "degree" not in kinds and input_dim == 5
    if method == 'VGRNN':
        assert isinstance(x_list, torch.Tensor) and tuple(x_list.shape) == (3, 5, 5)
    else:
        assert isinstance(x_list, list) and len(x_list) == 3
    if method == 'PGNN':
        assert dist_calls == [(3, 5, args["approximate"])] and node_dist_list == "dist"
    else:
        assert dist_calls == [] and node_dist_list is None


def test_degree_methods_read_feature_files_when_a_feature_folder_is_given_and_std_defaults(config):
    from ctgcn_amd import train
    args = dict(config["embedding"]["CTGCN-S"], origin_base_path="/o", core_base_path="/c", nfeature_path="/f", node_num=5)
    loader = StubLoader()
    train.get_input_data('CTGCN-S', 0, 2, loader, args)
    assert ("feature", "/f", 0, 2, False) in loader.calls and "degree" not in [c[0] for c in loader.calls]
    args = dict(config["embedding"]["EvolveGCN"], origin_base_path="/o", core_base_path=None, nfeature_path=None, node_num=5)
    del args["std"]
    loader = StubLoader()
    train.get_input_data('EvolveGCN', 0, 2, loader, args)
    assert ("degree", "/o", 0, 2, "\t", "gaussian", 1e-4) in loader.calls
    with pytest.raises(AssertionError):
        train.get_input_data('DynAE', 0, 2, loader, args)


def test_get_data_loader_resolves_the_paths_and_counts_the_snapshots(tmp_path):
    from ctgcn_amd import train
    (tmp_path / "origin").mkdir()
    (tmp_path / "cores").mkdir()
    for t in range(3):
        (tmp_path / "origin" / ("%d.csv" % t)).write_text("")
    for t in range(2):
        (tmp_path / "cores" / str(t)).mkdir()
    (tmp_path / "nodes.csv").write_text("a\nb\nc\nd\n")
    args = dict(base_path=str(tmp_path), origin_folder="origin", core_folder="cores", node_file="nodes.csv", has_cuda=False)
    loader = train.get_data_loader(args)
    assert loader.max_time_num == 3 and loader.full_node_list == ["a", "b", "c", "d"] and args["node_num"] == 4
    assert args["origin_base_path"] == str(tmp_path / "origin") and args["core_base_path"] == str(tmp_path / "cores")
    assert args["nfeature_path"] is None
    args = dict(base_path=str(tmp_path), origin_folder=None, core_folder="cores", node_file="nodes.csv", has_cuda=False)
    assert train.get_data_loader(args).max_time_num == 2 and args["origin_base_path"] is None


# ------------------------------------------------------------------------------------------------ get_gnn_model
CLASS_OF = {'CGCN-C': 'CGCN', 'CGCN-S': 'CGCN', 'CTGCN-C': 'CTGCN', 'CTGCN-S': 'CTGCN'}


@pytest.mark.parametrize("method", GNN)
def test_get_gnn_model_builds_every_method_from_the_uci_config(method, config):
    import ctgcn_amd
    from ctgcn_amd import train
    args = dict(config["embedding"][method], input_dim=37)
    model = train.get_gnn_model(method, 3, args)
    assert type(model) is getattr(ctgcn_amd, CLASS_OF.get(method, method))
    assert model.method_name == method
    assert (model.input_dim, model.hidden_dim, model.output_dim) == (37, args["hid_dim"], args["embed_dim"])
    if "dropout" in args and hasattr(model, "dropout"):
        assert model.dropout == args["dropout"]
    if "feature_dim" in args:
        assert (model.feature_dim, model.feature_pre, model.layer_num) == (args["feature_dim"], args["feature_pre"], args["layer_num"])
    if method == 'GAT':
        assert (model.head_num, model.alpha, model.learning_type) == (args["head_num"], args["alpha"], args["learning_type"])
    if method == 'SAGE':
        assert (model.num_sample, model.pooling_type) == (None, args["pooling_type"])
    if method == 'GIN':
        assert (model.layer_num, model.mlp_layer_num, model.learn_eps, model.neighbor_pooling_type) == (2, 2, False, 'sum')
    if method == 'VGRNN':
        assert (model.rnn_layer_num, model.conv_type) == (args["rnn_layer_num"], 'GCN')
    if method == 'EvolveGCN':
        assert model.egcn_type == args["model_type"]
    if method in CORE:
        assert (model.trans_num, model.diffusion_num) == (args["trans_layer_num"], args["diffusion_layer_num"])
        assert (model.model_type, model.rnn_type, model.trans_activate_type) == (args["model_type"], args["rnn_type"], args["trans_activate_type"])
    if method in ('CTGCN-C', 'CTGCN-S', 'GCRN'):
        assert model.duration == 3
        assert train.get_gnn_model(method, 2, args).duration == 2


def test_a_refused_model_option_surfaces_as_the_class_s_own_error(config):
    from ctgcn_amd import train
    args = dict(config["embedding"]["VGRNN"], input_dim=9, conv_type='SAGE')
    with pytest.raises(NotImplementedError, match="conv_type"):
        train.get_gnn_model('VGRNN', 2, args)
    args = dict(config["embedding"]["SAGE"], input_dim=9, num_sample=5)
    with pytest.raises(NotImplementedError):
        train.get_gnn_model('SAGE', 1, args)


# ------------------------------------------------------------------------------------------------ get_loss
class LabelLoader(object):
    def get_node_label_list(self, path, start_idx, duration, sep='\t'):
        return ["nl"] * duration, 4

    def get_edge_label_list(self, path, start_idx, duration, sep='\t'):
        return ["el"] * duration, 3

    def get_node_pair_list(self, path, start_idx, duration):
        return [[[1], [0]] for _ in range(duration)]

    def get_node_freq_list(self, path, start_idx, duration):
        return [[0, 1] for _ in range(duration)]


FAMILY = {'GCN': 'ClassificationLoss', 'CTGCN-C': 'ClassificationLoss', 'PGNN': 'ClassificationLoss', 'VGRNN': 'VAEClassificationLoss',
          'CGCN-S': 'StructureClassificationLoss', 'CTGCN-S': 'StructureClassificationLoss'}


@pytest.mark.parametrize("learning_type,cls_name,out_dim", [('S-node', 'MLPClassifier', 4), ('S-edge', 'EdgeClassifier', 3),
                                                            ('S-link-st', 'InnerProduct', 2), ('S-link-dy', 'InnerProduct', 2)])
@pytest.mark.parametrize("method", sorted(FAMILY))
def test_get_loss_supervised_types(method, learning_type, cls_name, out_dim, config, tmp_path):
    from ctgcn_amd import metrics, models, train
    args = dict(config["embedding"][method], base_path=str(tmp_path), learning_type=learning_type, nlabel_folder="nl", elabel_folder="el",
                cls_hid_dim=16, cls_layer_num=1, cls_bias=True, cls_activate_type='L')
    loss, classifier, node_labels, edge_labels = train.get_loss(method, 1, 2, LabelLoader(), args)
    assert type(loss) is getattr(metrics, FAMILY[method])
    assert getattr(loss, "classification_loss", loss).n_class == out_dim
    assert type(classifier) is getattr(models, cls_name)
    assert node_labels == (["nl", "nl"] if learning_type == 'S-node' else None)
    assert edge_labels == (["el", "el"] if learning_type == 'S-edge' else None)
    if cls_name != 'InnerProduct':
        head = classifier if cls_name == 'MLPClassifier' else classifier.classifier
        assert (head.input_dim, head.hidden_dim, head.output_dim) == (args["embed_dim"], 16, out_dim)
        assert (head.layer_num, head.duration, head.bias, head.activate_type) == (1, 2, True, 'L')


def test_get_loss_unsupervised_types(config, tmp_path, monkeypatch):
    from ctgcn_amd import metrics, train
    seen = {}

    class Neg(object):
        def __init__(self, pairs, freqs, neg_num=20, Q=10, seed=None):
            seen.update(pairs=pairs, freqs=freqs, neg_num=neg_num, Q=Q, seed=seed)

    monkeypatch.setattr(train, "NegativeSamplingLoss", Neg)
    args = dict(config["embedding"]["GCN"], base_path=str(tmp_path), Q=15)
    assert isinstance(train.get_loss('GCN', 2, 3, LabelLoader(), args), Neg)
    assert (seen["neg_num"], seen["Q"], seen["seed"], len(seen["pairs"]), len(seen["freqs"])) == (20, 15, None, 3, 3)
    train.get_loss('GCN', 2, 3, LabelLoader(), dict(args, seed=11))
    assert seen["seed"] == 11
    loss = train.get_loss('VGRNN', 0, 1, None, dict(config["embedding"]["VGRNN"], eps=1e-7))
    assert type(loss) is metrics.VAELoss and loss.eps == 1e-7
    for method in ('CGCN-S', 'CTGCN-S'):
        assert type(train.get_loss(method, 0, 1, None, dict(config["embedding"][method]))) is metrics.ReconstructionLoss
    for method in ('GCN', 'CTGCN-C', 'EvolveGCN'):
        with pytest.raises(NotImplementedError, match=method):
            train.get_loss(method, 0, 1, None, dict(config["embedding"][method], learning_type='U-own'))
    with pytest.raises(AssertionError):         # the UCI config's PGNN section says 'S-link', which the reference's get_loss refuses too
        train.get_loss('PGNN', 0, 1, None, dict(config["embedding"]["PGNN"]))


# ------------------------------------------------------------------------------------------------ preprocess
def test_preprocess_reads_the_reference_s_keys_and_the_seed(config, monkeypatch):
    from ctgcn_amd import preprocessing
    made = []

    class Structure(object):
        def __init__(self, *a):
            made.append(("structure",) + a)

        def get_kcore_graph_all_time(self, sep='\t', worker=-1):
            made.append(("kcore", sep, worker))

    class Walk(object):
        def __init__(self, *a, **k):
            made.append(("walk", a, k))

        def get_walk_info_all_time(self, worker=-1, sep='\t', weighted=True):
            made.append(("walks", worker, sep, weighted))

    monkeypatch.setattr(preprocessing, "StructureInfoGenerator", Structure)
    monkeypatch.setattr(preprocessing, "WalkGenerator", Walk)
    section = config["preprocessing"]
    preprocessing.preprocess('CTGCN-C', dict(section["CTGCN-C"], seed=5))
    assert made == [("structure", "/data/uci", "1.format", "CTGCN/ctgcn_cores", "nodes_set/nodes.csv"),
                    ("walk", ("/data/uci", "1.format", "CTGCN/ctgcn_walk_pairs", "CTGCN/ctgcn_node_freq", "nodes_set/nodes.csv"),
                     dict(walk_time=20, walk_length=5, seed=5)),
                    ("kcore", "\t", -1), ("walks", -1, "\t", True)]
    del made[:]
    preprocessing.preprocess('GCN', section["GCN"])                   # no core_folder: no structure generator; generate_core defaults False
    assert [m[0] for m in made] == ["walk", "walks"] and made[0][2]["seed"] is None and made[1] == ("walks", 30, "\t", True)
    del made[:]
    preprocessing.preprocess('CGCN-C', dict(section["CGCN-C"], generate_core=False, run_walk=False))
    assert [m[0] for m in made] == ["structure", "walk"]
    p = preprocessing.Processing("/b", "o", None, "w", "f", "n", 3, 4)
    assert p.structure_generator is None and made[-1] == ("walk", ("/b", "o", "w", "f", "n"), dict(walk_time=3, walk_length=4, seed=None))


# ------------------------------------------------------------------------------------------------ the command line
def _write_config(tmp_path, config):
    path = tmp_path / "config.json"
    path.write_text(json.dumps(config))
    return str(path)


def test_main_refuses_an_unknown_task_and_a_missing_method(tmp_path, config):
    from ctgcn_amd.main import main
    path = _write_config(tmp_path, config)
    with pytest.raises(AttributeError, match="task"):
        main(["prog", "--config", path, "--task", "train"])
    for task in ("preprocessing", "embedding"):
        with pytest.raises(AttributeError, match="method"):
            main(["prog", "--config", path, "--task", task])


def test_main_dispatches_every_task_to_its_entry_function(tmp_path, config, monkeypatch):
    import importlib
    import ctgcn_amd.baseline as baseline
    import ctgcn_amd.preprocessing as preprocessing
    # import_module: the package exports functions that carry their submodules' names
    cp, ec, lp, nc, sp = (importlib.import_module("ctgcn_amd.evaluation." + name) for name in
                          ("centrality_prediction", "edge_classification", "link_prediction", "node_classification", "similarity_prediction"))
    import ctgcn_amd.train as train
    from ctgcn_amd.main import main
    config = copy.deepcopy(config)
    config["node_cls"] = {"marker": "node"}
    config["edge_cls"] = {"marker": "edge"}
    config["embedding"]["GCN"]["use_cuda"] = True
    del config["embedding"]["CTGCN-C"]["use_cuda"]
    path = _write_config(tmp_path, config)
    calls = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(baseline, "dyngem_embedding", lambda method, args: calls.append(("dyngem", method, args)))
    monkeypatch.setattr(baseline, "timers_embedding", lambda args: calls.append(("timers", None, args)))
    monkeypatch.setattr(train, "gnn_embedding", lambda method, args: calls.append(("gnn", method, args)))
    monkeypatch.setattr(preprocessing, "preprocess", lambda method, args: calls.append(("preprocess", method, args)))
    for mod, name in ((lp, "link_prediction"), (nc, "node_classification"), (ec, "edge_classification"), (cp, "centrality_prediction"),
                      (sp, "similarity_prediction")):
        monkeypatch.setattr(mod, name, lambda args, name=name: calls.append((name, None, args)))
    before = dict(os.environ)
    for method in NON_GNN + GNN:
        del calls[:]
        main(["prog", "--config", path, "--task", "embedding", "--method", method])
        want = "dyngem" if method in NON_GNN[:4] else "timers" if method == 'TIMERS' else "gnn"
        assert len(calls) == 1 and calls[0][0] == want and calls[0][1] == (None if want == "timers" else method)
        args = calls[0][2]
        assert args["has_cuda"] is True and args["base_path"] == "/data/uci"
        assert {k: v for k, v in args.items() if k != "has_cuda"} == config["embedding"][method]
    del calls[:]
    main(["prog", "--config", path, "--task", "preprocessing", "--method", "CTGCN-C"])
    assert calls == [("preprocess", "CTGCN-C", config["preprocessing"]["CTGCN-C"])]
    with pytest.raises(AssertionError):
        main(["prog", "--config", path, "--task", "preprocessing", "--method", "CTGCN-S"])
    for task, name in (("link_pred", "link_prediction"), ("node_cls", "node_classification"), ("edge_cls", "edge_classification"),
                       ("cent_pred", "centrality_prediction"), ("sim_pred", "similarity_prediction")):
        del calls[:]
        main(["prog", "--config", path, "--task", task])
        assert calls == [(name, None, config[task])]
    assert dict(os.environ) == before


def test_the_embedding_task_needs_a_gpu_and_leaves_the_environment_alone(tmp_path, config, monkeypatch):
    import ctgcn_amd.train as train
    from ctgcn_amd import CtgcnHipError
    from ctgcn_amd.main import main
    config = copy.deepcopy(config)
    config["embedding"]["GAT"]["use_cuda"] = False
    del config["embedding"]["GIN"]["use_cuda"]
    path = _write_config(tmp_path, config)
    reached = []
    monkeypatch.setattr(train, "gnn_embedding", lambda method, args: reached.append(method))
    monkeypatch.setattr(train, "get_data_loader", lambda args: reached.append("loader"))
    before = dict(os.environ)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for method in ("GCN", "GIN", "DynGEM", "TIMERS"):
        with pytest.raises(CtgcnHipError, match="torch.cuda.is_available"):
            main(["prog", "--config", path, "--task", "embedding", "--method", method])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(CtgcnHipError, match="use_cuda is false"):
        main(["prog", "--config", path, "--task", "embedding", "--method", "GAT"])
    assert reached == [] and dict(os.environ) == before
    source = open(os.path.join(os.path.dirname(train.__file__), "main.py")).read()
    assert "environ[" not in source and "putenv" not in source


def test_the_module_runs_as_a_command(tmp_path, config):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = _write_config(tmp_path, config)
    run = subprocess.run([sys.executable, "-m", "ctgcn_amd.main", "--config", path, "--task", "embedding"], cwd=root, capture_output=True,
                         text=True)
    assert run.returncode != 0 and "AttributeError" in run.stderr and "method" in run.stderr
    run = subprocess.run([sys.executable, "-m", "ctgcn_amd.main", "--task", "embedding"], cwd=root, capture_output=True, text=True)
    assert run.returncode == 2 and "--config" in run.stderr


def test_ctgcn_hip_error_is_exported():
    import ctgcn_amd
    from ctgcn_amd._lib import CtgcnHipError
    assert ctgcn_amd.CtgcnHipError is CtgcnHipError


# ------------------------------------------------------------------------------------------------ the trainers and GCN
def test_the_trainers_take_this_package_s_gcn_and_no_other_module_of_that_name():
    from ctgcn_amd import baseline, embedding, metrics
    assert "GCN" not in embedding._SUPPORTED and embedding._MODULE_TRAINED == ('GCN',)

    class Other(torch.nn.Module):
        method_name = "GCN"

    unsup = object.__new__(embedding.UnsupervisedEmbedding)
    unsup.loss = metrics.NegativeSamplingLoss.__new__(metrics.NegativeSamplingLoss)
    sup = object.__new__(embedding.SupervisedEmbedding)
    sup.loss = metrics.ClassificationLoss(2)
    own = baseline.GCN(6, 4, 3)
    for trainer in (unsup, sup):
        assert trainer._check_model(own) == "GCN"
        with pytest.raises(NotImplementedError, match="GCN"):
            trainer._check_model(Other())
        relabelled = baseline.EvolveGCN(6, 4, 3)
        relabelled.method_name = "GCN"
        with pytest.raises(NotImplementedError):
            trainer._check_model(relabelled)
        with pytest.raises(NotImplementedError):
            trainer._check_model(torch.nn.Linear(2, 2))
    sup.loss = metrics.StructureClassificationLoss(2)
    with pytest.raises(ValueError, match="ClassificationLoss"):
        sup._check_model(own)


def test_the_driver_entries_are_exported():
    import ctgcn_amd
    from ctgcn_amd import baseline
    from ctgcn_amd.baseline import dynae
    assert ctgcn_amd.dyngem_embedding is baseline.dyngem_embedding is dynae.dyngem_embedding
    assert ctgcn_amd.gnn_embedding is ctgcn_amd.train.gnn_embedding
    for name in ("dyngem_embedding", "gnn_embedding", "window_schedule"):
        assert name in ctgcn_amd.__all__


def test_dyngem_embedding_makes_the_reference_s_assertions(tmp_path, config):
    from ctgcn_amd import dyngem_embedding
    (tmp_path / "1.format").mkdir()
    (tmp_path / "nodes_set").mkdir()
    for t in range(4):
        (tmp_path / "1.format" / ("%d.csv" % t)).write_text("from_id\tto_id\n")
    (tmp_path / "nodes_set" / "nodes.csv").write_text("a\nb\n")
    base = dict(base_path=str(tmp_path), has_cuda=True)
    with pytest.raises(AssertionError):
        dyngem_embedding('GCN', dict(config["embedding"]["GCN"], **base))
    with pytest.raises(AssertionError):                                     # DynGEM: duration == 1
        dyngem_embedding('DynGEM', dict(config["embedding"]["DynGEM"], duration=2, **base))
    with pytest.raises(AssertionError):                                     # start_idx + 1 - duration >= 0
        dyngem_embedding('DynAE', dict(config["embedding"]["DynAE"], start_idx=1, **base))
    with pytest.raises(AssertionError):                                     # duration > look_back
        dyngem_embedding('DynRNN', dict(config["embedding"]["DynRNN"], look_back=3, **base))
    with pytest.raises(KeyError):                                           # DynAERNN reads ae_units and rnn_units, not n_units
        dyngem_embedding('DynAERNN', dict(config["embedding"]["DynRNN"], **base))
