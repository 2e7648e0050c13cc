"""The command line of the package, the reference's main.py:

    python -m ctgcn_amd.main --config <json> --task <task> [--method <name>]

task is one of preprocessing, embedding, link_pred, node_cls, edge_cls, cent_pred, sim_pred, graph_recon; the config file has the
reference's schema (config/*.json: one section per task, and per method under 'preprocessing' and 'embedding').  graph_recon (MAP and
precision@k over a ranking of all node pairs, evaluation/graph_reconstruction.py) and its config section are this package's own
extension: the reference has neither.  The embedding task runs on the MI355X only:
without a visible GPU, or with use_cuda false, it raises CtgcnHipError before anything is loaded.  Unlike the reference this module
never touches os.environ: which devices a run sees is the caller's choice.
"""
import argparse
import json
import sys

import torch

from ._lib import CtgcnHipError
from .utils import get_supported_methods

TASKS = ('preprocessing', 'embedding', 'link_pred', 'node_cls', 'edge_cls', 'cent_pred', 'sim_pred', 'graph_recon')
_PREPROCESSED = ('GCN', 'GCN_TG', 'GAT', 'GAT_TG', 'SAGE', 'SAGE_TG', 'GIN', 'GIN_TG', 'PGNN', 'CGCN-C', 'GCRN', 'EvolveGCN', 'CTGCN-C')


def parse_args(args):
    parser = argparse.ArgumentParser(prog='CTGCN', description='K-core based Temporal Graph Convolutional Network')
    parser.add_argument('--config', nargs=1, type=str, help='configuration file path', required=True)
    parser.add_argument('--task', type=str, default='embedding', help='task name which is needed to run', required=True)
    parser.add_argument('--method', type=str, default=None, help='graph embedding method, only used for the preprocessing and embedding tasks')
    return parser.parse_args(args)


def parse_json_args(file_path):
    with open(file_path) as config_file:
        return json.load(config_file)


def preprocessing_task(method, args):
    """CGCN-S and CTGCN-S train on their own loss and need no walk corpus: they have no preprocessing section"""
    from .preprocessing import preprocess
    assert method in _PREPROCESSED
    preprocess(method, args[method])


def embedding_task(method, args):
    print(args)
    assert method in get_supported_methods()
    args['has_cuda'] = bool(torch.cuda.is_available())
    if 'use_cuda' in args:
        if args['use_cuda'] and not args['has_cuda']:
            raise CtgcnHipError("the embedding task runs on the MI355X only: use_cuda is set but torch.cuda.is_available() is False "
                                "(no GPU is visible to this process); there is no CPU fallback")
        args['has_cuda'] &= bool(args['use_cuda'])
    if not args['has_cuda']:
        reason = "use_cuda is false in the config" if torch.cuda.is_available() else "torch.cuda.is_available() is False (no GPU is visible)"
        raise CtgcnHipError("the embedding task runs on the MI355X only: %s; there is no CPU fallback" % reason)

    from .baseline import dyngem_embedding, timers_embedding
    from .train import gnn_embedding
    if method in ['DynGEM', 'DynAE', 'DynRNN', 'DynAERNN']:
        dyngem_embedding(method, args)
    elif method == 'TIMERS':
        timers_embedding(args)
    else:
        gnn_embedding(method, args)


def link_prediction_task(args):
    from .evaluation.link_prediction import link_prediction
    link_prediction(args)


def node_classification_task(args):
    from .evaluation.node_classification import node_classification
    node_classification(args)


def edge_classification_task(args):
    from .evaluation.edge_classification import edge_classification
    edge_classification(args)


def centrality_prediction_task(args):
    from .evaluation.centrality_prediction import centrality_prediction
    centrality_prediction(args)


def similarity_prediction_task(args):
    from .evaluation.similarity_prediction import similarity_prediction
    similarity_prediction(args)


def graph_reconstruction_task(args):
    from .evaluation.graph_reconstruction import graph_reconstruction
    graph_reconstruction(args)


_EVALUATION_TASKS = {'link_pred': link_prediction_task, 'node_cls': node_classification_task, 'edge_cls': edge_classification_task,
                     'cent_pred': centrality_prediction_task, 'sim_pred': similarity_prediction_task,
                     'graph_recon': graph_reconstruction_task}


def main(argv):
    """argv as sys.argv: argv[0] is the program name"""
    args = parse_args(argv[1:])
    print('args:', args)
    if args.task not in TASKS:
        raise AttributeError('Unsupported task!')
    if args.task in ('preprocessing', 'embedding') and args.method is None:
        raise AttributeError('Embedding method parameter is needed for the %s task!' % args.task)
    config_dict = parse_json_args(args.config[0])
    args_dict = config_dict[args.task]
    if args.task == 'preprocessing':
        preprocessing_task(args.method, args_dict)
    elif args.task == 'embedding':
        embedding_task(args.method, args_dict[args.method])
    else:
        _EVALUATION_TASKS[args.task](args_dict)


if __name__ == '__main__':
    main(sys.argv)
