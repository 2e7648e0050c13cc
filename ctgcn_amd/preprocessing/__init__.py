"""Processing and preprocess(method, args): the reference's preprocessing entry (reference preprocessing/__init__.py) over this
package's generators.  `seed` is the one key the reference does not have: it goes to WalkGenerator(seed=...)."""
import time

from .structure_generation import StructureInfoGenerator  # noqa: F401
from .walk_generation import WalkGenerator  # noqa: F401


class Processing(object):
    def __init__(self, base_path, origin_folder, core_folder, walk_pair_folder, node_freq_folder, node_file, walk_time=100, walk_length=5,
                 seed=None):
        self.structure_generator = None
        if core_folder is not None:
            self.structure_generator = StructureInfoGenerator(base_path, origin_folder, core_folder, node_file)
        self.walk_generator = WalkGenerator(base_path, origin_folder, walk_pair_folder, node_freq_folder, node_file, walk_time=walk_time,
                                            walk_length=walk_length, seed=seed)

    def run(self, worker=-1, generate_core=True, run_walk=True, sep='\t', weighted=True):
        if self.structure_generator is not None and generate_core:
            t1 = time.time()
            print('start generate k core graph!')
            self.structure_generator.get_kcore_graph_all_time(sep=sep, worker=worker)
            print('finish generate k core graph! cost time:', time.time() - t1, 'seconds!')
        if run_walk:
            t1 = time.time()
            print('start generate walk info!')
            self.walk_generator.get_walk_info_all_time(worker=worker, sep=sep, weighted=weighted)
            print('finish generate walk info! cost time: ', time.time() - t1, ' seconds.')


def preprocess(method, args):
    """The preprocessing task of one method's config section: k-core files (when core_folder is given and generate_core is set) and the
    walk corpus."""
    t1 = time.time()
    processing = Processing(base_path=args['base_path'], origin_folder=args['origin_folder'], core_folder=args.get('core_folder', None),
                            walk_pair_folder=args['walk_pair_folder'], node_freq_folder=args['node_freq_folder'], node_file=args['node_file'],
                            walk_time=args['walk_time'], walk_length=args['walk_length'], seed=args.get('seed', None))
    processing.run(worker=args['worker'], generate_core=args.get('generate_core', False), run_walk=args.get('run_walk', True),
                   sep=args['file_sep'], weighted=args['weighted'])
    print('finish ' + method + ' preprocessing! total cost time:', time.time() - t1, ' seconds!')
