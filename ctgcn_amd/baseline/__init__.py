"""Methods CTGCN is compared against (the reference's `baseline` package), on the same HIP library."""
from .egcn import EvolveGCN  # noqa: F401
