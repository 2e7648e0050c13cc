"""The GNN driver: the reference's train.py (get_data_loader, get_input_data, get_gnn_model, get_loss, gnn_embedding) over this
package's loaders, models, losses and trainers, with the reference's names, argument order and return shapes.  It reads the reference's
config schema (a method's section of config/*.json) and adds no device path of its own.

What a method gets (get_input_data):
    core lists      core-based methods: get_core_adj_list(core_base_path, max_core=args['max_core']) is their adj_list
    adjacency       get_date_adj_list(normalize, row_norm, add_eye), always data_type='tensor':
                    GCN, GAT, GCRN (True, True, True); EvolveGCN (True, False, True); every other method (False, False, False)
    edge_list       [adj._indices() for adj in ...] of that call, for every method (so it holds the self loops wherever add_eye is set)
    adj_list None   TgGCN, TgGAT, TgSAGE, TgGIN, PGNN
    features        EvolveGCN, CGCN-S, CTGCN-S without a feature folder: get_degree_feature_list(init_type, std); every other method
                    get_feature_list(nfeature_path, shuffle=False)
    VGRNN           x_list is stacked into one tensor, as the reference passes it (torch stacks sparse identities; the model reads
                    x_list[t] of a list or of a stack)
    PGNN            node_dist_list = baseline.pgnn.precompute_dist_data(edge_list, node_num, approximate=args['approximate'])

`seed` is the one key the reference does not have.  With it gnn_embedding seeds torch, numpy.random and random before each window,
builds NegativeSamplingLoss(seed=seed) and passes seed to SupervisedEmbedding.learn_embedding, so two runs write the same bytes;
without it the entropy comes from the OS, as in the reference.
"""
import os
import random
import time

import numpy as np
import pandas as pd
import torch

from .embedding import SupervisedEmbedding, UnsupervisedEmbedding
from .helper import DataLoader
from .metrics import (ClassificationLoss, NegativeSamplingLoss, ReconstructionLoss, StructureClassificationLoss, VAEClassificationLoss,
                      VAELoss)
from .models import CGCN, CTGCN, EdgeClassifier, InnerProduct, MLPClassifier
from .utils import get_core_based_methods, get_supported_gnn_methods

LEARNING_TYPES = ('U-neg', 'U-own', 'S-node', 'S-edge', 'S-link-st', 'S-link-dy')
_ROW_NORMALISED = ('GCN', 'GAT', 'GCRN')            # D^-1 (A + I)
_SYM_NORMALISED = ('EvolveGCN',)                    # D^-1/2 (A + I) D^-1/2
_NO_ADJACENCY = ('TgGCN', 'TgGAT', 'TgSAGE', 'TgGIN', 'PGNN')
_DEGREE_FEATURES = ('EvolveGCN', 'CGCN-S', 'CTGCN-S')
_S_MODELS = ('CGCN-S', 'CTGCN-S')


def get_data_loader(args):
    base_path = args['base_path']
    origin_folder = args['origin_folder']
    core_folder = args.get('core_folder', None)
    nfeature_folder = args.get('nfeature_folder', None)

    node_path = os.path.abspath(os.path.join(base_path, args['node_file']))
    node_list = pd.read_csv(node_path, names=['node'])['node'].tolist()

    origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder)) if origin_folder else None
    core_base_path = os.path.abspath(os.path.join(base_path, core_folder)) if core_folder else None
    node_feature_path = os.path.abspath(os.path.join(base_path, nfeature_folder)) if nfeature_folder else None
    max_time_num = len(os.listdir(origin_base_path)) if origin_base_path else len(os.listdir(core_base_path))
    assert max_time_num > 0

    data_loader = DataLoader(node_list, max_time_num, has_cuda=args['has_cuda'])
    args['origin_base_path'] = origin_base_path
    args['core_base_path'] = core_base_path
    args['nfeature_path'] = node_feature_path
    args['node_num'] = len(node_list)
    return data_loader


def adjacency_normalisation(method):
    """(normalize, row_norm, add_eye) of a method's get_date_adj_list call"""
    if method in _ROW_NORMALISED:
        return True, True, True
    if method in _SYM_NORMALISED:
        return True, False, True
    return False, False, False


def get_input_data(method, idx, time_length, data_loader, args):
    """(input_dim, adj_list, x_list, edge_list, node_dist_list) of the window idx .. idx + time_length - 1; the rules are in the
    module's docstring"""
    assert method in get_supported_gnn_methods()
    origin_base_path = args['origin_base_path']
    node_feature_path = args['nfeature_path']
    file_sep = args['file_sep']

    core_adj_list = []
    if method in get_core_based_methods():
        core_adj_list = data_loader.get_core_adj_list(args['core_base_path'], start_idx=idx, duration=time_length, max_core=args['max_core'])
    normalize, row_norm, add_eye = adjacency_normalisation(method)
    adj_list = data_loader.get_date_adj_list(origin_base_path, start_idx=idx, duration=time_length, sep=file_sep, normalize=normalize,
                                             row_norm=row_norm, add_eye=add_eye, data_type='tensor')
    edge_list = [adj._indices() for adj in adj_list]        # every method needs it for the S-link learning types

    if method in get_core_based_methods():
        adj_list = core_adj_list
    elif method in _NO_ADJACENCY:
        adj_list = None

    if method in _DEGREE_FEATURES and node_feature_path is None:
        x_list, input_dim = data_loader.get_degree_feature_list(origin_base_path, start_idx=idx, duration=time_length, sep=file_sep,
                                                                init_type=args['init_type'], std=args.get('std', 1e-4))
    else:
        x_list, input_dim = data_loader.get_feature_list(node_feature_path, start_idx=idx, duration=time_length, shuffle=False)
        if method == 'VGRNN':
            x_list = torch.stack(x_list)

    node_dist_list = None
    if method == 'PGNN':
        from .baseline import pgnn
        node_dist_list = pgnn.precompute_dist_data(edge_list, args['node_num'], approximate=args['approximate'])
    return input_dim, adj_list, x_list, edge_list, node_dist_list


def get_gnn_model(method, time_length, args):
    """This package's model of `method` from the reference's keys.  An option a class refuses (SAGE num_sample, VGRNN conv_type, ...)
    surfaces as that class's own error."""
    assert method in get_supported_gnn_methods()
    from . import baseline

    input_dim = args['input_dim']
    hidden_dim = args['hid_dim']
    embed_dim = args['embed_dim']
    dropout = args.get('dropout', None)
    bias = args.get('bias', None)

    if method == 'GCN':
        return baseline.GCN(input_dim, hidden_dim, embed_dim, dropout=dropout, bias=bias)
    if method == 'GAT':
        return baseline.GAT(input_dim, hidden_dim, embed_dim, dropout=dropout, alpha=args['alpha'], head_num=args['head_num'],
                            learning_type=args['learning_type'])
    if method == 'SAGE':
        return baseline.SAGE(input_dim, hidden_dim, embed_dim, num_sample=args['num_sample'], pooling_type=args['pooling_type'], gcn=False,
                             dropout=dropout, bias=bias)
    if method == 'GIN':
        return baseline.GIN(input_dim, hidden_dim, embed_dim, args['layer_num'], args['mlp_layer_num'], args['learn_eps'], args['pooling_type'],
                            dropout=dropout, bias=bias)
    if method in ('TgGCN', 'TgGAT', 'TgSAGE', 'TgGIN', 'PGNN', 'GCRN'):
        kwargs = dict(feature_pre=args['feature_pre'], layer_num=args['layer_num'], dropout=dropout, bias=bias)
        if method == 'GCRN':
            kwargs.update(duration=time_length, rnn_type=args['rnn_type'])
        return getattr(baseline, method)(input_dim, args['feature_dim'], hidden_dim, embed_dim, **kwargs)
    if method == 'VGRNN':
        return baseline.VGRNN(input_dim, hidden_dim, embed_dim, rnn_layer_num=args['rnn_layer_num'], conv_type=args['conv_type'], bias=bias)
    if method == 'EvolveGCN':
        return baseline.EvolveGCN(input_dim, hidden_dim, embed_dim, egcn_type=args['model_type'])
    # the core-based models, static and temporal
    kwargs = dict(trans_num=args['trans_layer_num'], diffusion_num=args['diffusion_layer_num'], bias=bias, rnn_type=args['rnn_type'],
                  model_type=args['model_type'], trans_activate_type=args['trans_activate_type'])
    if method in ('CGCN-C', 'CGCN-S'):
        return CGCN(input_dim, hidden_dim, embed_dim, **kwargs)
    return CTGCN(input_dim, hidden_dim, embed_dim, duration=time_length, **kwargs)


def get_loss(method, idx, time_length, data_loader, args):
    """The loss of an unsupervised learning type, or (loss, classifier, node_label_list, edge_label_list) of a supervised one"""
    learning_type = args['learning_type']
    assert learning_type in LEARNING_TYPES
    base_path = args['base_path']
    file_sep = args['file_sep']

    if learning_type == 'U-neg':
        walk_pair_base_path = os.path.abspath(os.path.join(base_path, args['walk_pair_folder']))
        node_freq_base_path = os.path.abspath(os.path.join(base_path, args['node_freq_folder']))
        node_pair_list = data_loader.get_node_pair_list(walk_pair_base_path, start_idx=idx, duration=time_length)
        neg_freq_list = data_loader.get_node_freq_list(node_freq_base_path, start_idx=idx, duration=time_length)
        return NegativeSamplingLoss(node_pair_list, neg_freq_list, neg_num=args['neg_num'], Q=args['Q'], seed=args.get('seed', None))
    if learning_type == 'U-own':
        if method == 'VGRNN':
            return VAELoss(eps=args['eps'])
        if method in _S_MODELS:
            return ReconstructionLoss()
        raise NotImplementedError('No implementation of ' + method + '\'s unsupervised learning loss!')

    embed_dim = args['embed_dim']
    cls_hidden_dim = args.get('cls_hid_dim', None)
    cls_layer_num = args.get('cls_layer_num', None)
    cls_bias = args.get('cls_bias', None)
    cls_activate_type = args.get('cls_activate_type', None)
    node_label_list, edge_label_list = None, None
    if learning_type == 'S-node':
        nlabel_base_path = os.path.abspath(os.path.join(base_path, args['nlabel_folder']))
        node_label_list, output_dim = data_loader.get_node_label_list(nlabel_base_path, start_idx=idx, duration=time_length, sep=file_sep)
        classifier = MLPClassifier(embed_dim, cls_hidden_dim, output_dim, layer_num=cls_layer_num, duration=time_length, bias=cls_bias,
                                   activate_type=cls_activate_type)
    elif learning_type == 'S-edge':
        elabel_base_path = os.path.abspath(os.path.join(base_path, args['elabel_folder']))
        edge_label_list, output_dim = data_loader.get_edge_label_list(elabel_base_path, start_idx=idx, duration=time_length, sep=file_sep)
        classifier = EdgeClassifier(embed_dim, cls_hidden_dim, output_dim, layer_num=cls_layer_num, duration=time_length, bias=cls_bias,
                                    activate_type=cls_activate_type)
    else:       # S-link-st, S-link-dy
        classifier = InnerProduct()
        output_dim = 2      # positive link and negative link
    if method == 'VGRNN':
        loss = VAEClassificationLoss(output_dim, eps=args['eps'])
    elif method in _S_MODELS:
        loss = StructureClassificationLoss(output_dim)
    else:
        loss = ClassificationLoss(output_dim)
    return loss, classifier, node_label_list, edge_label_list


def resolve_range(max_time_num, start_idx, end_idx):
    """[start, end) of the configured range: a negative start_idx counts from the end; end_idx is inclusive, negative from the end"""
    if start_idx < 0:
        start_idx = max_time_num + start_idx
    end_idx = max_time_num + end_idx + 1 if end_idx < 0 else end_idx + 1
    return start_idx, end_idx


def window_schedule(max_time_num, start_idx, end_idx, duration, learning_type):
    """[(idx, time_length)] of the window loop (reference train.py:253-271).  S-link-dy scores snapshot t + 1 against the embedding of
    t: the last snapshot is no input, and consecutive windows share one snapshot (step duration - 1)."""
    start_idx, end_idx = resolve_range(max_time_num, start_idx, end_idx)
    step = duration
    if learning_type == 'S-link-dy':
        assert duration >= 2 and end_idx - start_idx >= 1
        end_idx = end_idx - 1
        step = duration - 1
    return [(idx, min(idx + duration, end_idx) - idx) for idx in range(start_idx, end_idx, step)]


def seed_everything(seed):
    """torch, numpy.random and random from one seed (the driver's `seed` key); None leaves them alone"""
    if seed is None:
        return
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed % (2 ** 32))
    random.seed(seed)


def write_time_file(base_path, method, time_list):
    """<base_path>/<method>_time.csv: one `time` column, one row per window"""
    pd.DataFrame({'time': time_list}).to_csv(os.path.join(base_path, method + '_time.csv'), sep=',', index=False)


def gnn_embedding(method, args):
    base_path = args['base_path']
    origin_folder = args['origin_folder']
    embedding_folder = args['embed_folder']
    model_folder = args['model_folder']
    model_file = args['model_file']
    duration = args['duration']
    has_cuda = args['has_cuda']
    learning_type = args['learning_type']
    epoch = args['epoch']
    lr = args['lr']
    batch_size = args['batch_size']
    load_model = args['load_model']
    shuffle = args['shuffle']
    export = args['export']
    record_time = args['record_time']
    weight_decay = args['weight_decay']
    seed = args.get('seed', None)

    data_loader = get_data_loader(args)
    node_list = data_loader.full_node_list
    schedule = window_schedule(data_loader.max_time_num, args['start_idx'], args['end_idx'], duration, learning_type)

    t1 = time.time()
    time_list = []
    print('start ' + method + ' embedding! windows (idx, time_length):', schedule)
    for idx, time_length in schedule:
        print('idx = ', idx, ', duration = ', duration)
        seed_everything(seed)
        input_dim, adj_list, x_list, edge_list, node_dist_list = get_input_data(method, idx, time_length, data_loader, args)
        args['input_dim'] = input_dim
        model = get_gnn_model(method, time_length, args)

        if learning_type in ['U-neg', 'U-own']:
            loss = get_loss(method, idx, time_length, data_loader, args)
            trainer = UnsupervisedEmbedding(base_path=base_path, origin_folder=origin_folder, embedding_folder=embedding_folder,
                                            node_list=node_list, model=model, loss=loss, model_folder=model_folder, has_cuda=has_cuda)
            cost_time = trainer.learn_embedding(adj_list, x_list, edge_list, node_dist_list, epoch=epoch, batch_size=batch_size, lr=lr,
                                                start_idx=idx, weight_decay=weight_decay, model_file=model_file, load_model=load_model,
                                                shuffle=shuffle, export=export)
        else:
            loss, classifier, node_labels, edge_labels = get_loss(method, idx, time_length, data_loader, args)
            trainer = SupervisedEmbedding(base_path=base_path, origin_folder=origin_folder, embedding_folder=embedding_folder,
                                          node_list=node_list, model=model, loss=loss, classifier=classifier, model_folder=model_folder,
                                          has_cuda=has_cuda)
            cost_time = trainer.learn_embedding(adj_list, x_list, node_labels, edge_labels, edge_list, node_dist_list,
                                                learning_type=learning_type, epoch=epoch, batch_size=batch_size, lr=lr, start_idx=idx,
                                                weight_decay=weight_decay, train_ratio=args['train_ratio'], val_ratio=args['val_ratio'],
                                                test_ratio=args['test_ratio'], model_file=model_file, classifier_file=args.get('cls_file', None),
                                                load_model=load_model, shuffle=shuffle, export=export, seed=seed)
        time_list.append(cost_time)

    if record_time:
        write_time_file(base_path, method, time_list)
    print('finish ' + method + ' embedding! cost time: ', time.time() - t1, ' seconds!')
