"""drtk.utils.indexing of the drop-in (drtk/utils/indexing.py of the reference)."""
from drtk_amd.geometry import index  # noqa: F401
