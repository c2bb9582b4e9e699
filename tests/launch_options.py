"""One way for tests to set library options (tr_set_option): `with options(steal=2, grid_nodes=0): ...` sets the
named options and, on the way out, puts EVERY option back to the library's default -- so a test that fails half-way
leaves no non-default launch path behind for the tests after it.

DEFAULTS restates the initialisers of `struct tr_options` (csrc/tr_internal.h); tests/test_kernel_inventory.py parses
the header and fails when the two disagree."""
import contextlib

DEFAULTS = {
    "adaptive": 1, "compact": 1, "xcd_chunk": 128, "steal": 1, "tile": 1, "tile_small": 4, "node_layout": 1,
    "build_cache": 1, "stream": 1, "stream_rays": 256, "stream_refill": 0, "stream_dynamic": 1, "grid_nodes": 1,
    "split": 1, "split_steal": 8, "split_outlier": 1, "split_floor": 40, "leaf_vote": 32, "order_transfer": 1,
    "sort_inline": 1, "wide": 2, "wide_direct": 1, "wide_stack": 12, "expand_cus": 0, "expand_tiles": 1, "usteal": 1,
}


def restore_defaults():
    import triro.backend.ops as hops
    for name, value in DEFAULTS.items():
        hops.set_option(name, value)


@contextlib.contextmanager
def options(**kw):
    """set the given options (live names only) for the body; restore every option to DEFAULTS afterwards"""
    import triro.backend.ops as hops
    bad = [k for k in kw if k not in DEFAULTS]
    if bad:
        raise KeyError(f"not a live option: {bad}")
    try:
        for name, value in kw.items():
            hops.set_option(name, value)
        yield
    finally:
        restore_defaults()
