"""syzgydb_amd -- MI355X-native brute-force vector scan behind SyzgyDB's
Collection.Search.  The compute lives in libsyzgy_scan.so
(hand-written HIP for gfx950, C ABI in include/syzgy_scan.h); this package is
the host-side mirror of the reference's API for that path.
"""
from ._lib import (SZG_COSINE, SZG_EUCLIDEAN, SzgError, LIB_PATH)  # noqa: F401
from .index import ScanIndex, ScanMask, ScanColumn, pack_allow_bits, f64_probe, scan_plan, scan_group_plan, scan_matrix_plan, scan_select_plan, scan_wide_plan, reorder_plan, bulk_plan, option_check  # noqa: F401
from .collection import (Collection, CollectionOptions, Document, SearchArgs, SearchResult,  # noqa: F401
                         SearchResults, Euclidean, Cosine)
from . import codec  # noqa: F401
from . import regex_dfa  # noqa: F401
from . import where  # noqa: F401
from .where import Field  # noqa: F401
from . import lsh  # noqa: F401
from .pager import SpanfilePager  # noqa: F401

__all__ = ["ScanIndex", "ScanMask", "ScanColumn", "Field", "where", "regex_dfa", "Collection", "CollectionOptions", "Document", "SearchArgs",
           "SearchResult", "SearchResults", "Euclidean", "Cosine", "codec", "SzgError",
           "pack_allow_bits", "f64_probe", "scan_plan", "scan_group_plan", "scan_matrix_plan", "scan_select_plan", "scan_wide_plan", "reorder_plan", "bulk_plan", "option_check", "SpanfilePager", "lsh", "SZG_COSINE", "SZG_EUCLIDEAN", "LIB_PATH"]
