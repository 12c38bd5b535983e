"""The inputs over which a pm_run's launch sequence is pinned down, shared by
tools/run_launch_counts.py (which records tests/golden/run_launch_counts.json on a GPU),
tests/test_gpu_launch_counts.py (the built library against that file) and
tests/test_schedule_host.py (pm_schedule.cpp against it, without a GPU).

trees x option configurations x (2049 sites = 2 tiles, 33 sites = 1 tile) x (every leaf present,
one leaf absent at one site) x the four modes.  An entry is COUNTS: the timer spans of the
post-order, pre-order and tail classes and the run's run.* phase values (-1: not logged)."""
import json
import os

import numpy as np

import _shapes
from test_gpu_paths import CONFIGS as _PATH_CONFIGS
from test_gpu_paths import DEFAULTS as _PATH_DEFAULTS
from test_plan_host import tree_set

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_launch_counts.json")
MODES = (0, 1, 2, 3)   # PM_MODE_FITCH, SANKOFF, BLOCK_FITCH, BLOCK_SANKOFF
SITES = (2049, 33)
PRESENT = (True, False)
TIMER_CLASSES = (0, 1, 5)
PHASES = ("run.nt_loads", "run.down_pack", "run.down_pack_launches", "run.tail_pack", "run.tail_s_waves")
COUNTS = tuple(f"launches_{k}" for k in TIMER_CLASSES) + PHASES

DEFAULTS = dict(_PATH_DEFAULTS, tail_pack=1, down_pack=1)
CONFIGS = [(name, cfg) for name, cfg, _ in _PATH_CONFIGS if "graph" not in cfg and "nt" not in cfg] + [
    ("tail_pack_always", dict(tail_pack=-1)),
    ("down_pack_always", dict(down_pack=-1)),
    ("plain_min_waves2", dict(plain_up=(True, 2))),
    ("sub_down", dict(sub_down=True)),
    ("no_bands_no_groups", dict(narrow=0, group=(0, 4))),
]


def full(cfg):
    return {**DEFAULTS, **cfg}


def option_values(cfg):
    """The configuration as pm_set_option values: cluster, narrow, group waves, group levels,
    up_group, plain_up, sub_down, tail_pack, down_pack, subtree, virtual."""
    c = full(cfg)
    on, waves = c["plain_up"]
    plain = (int(waves) if waves >= 2 else 1) if on else 0
    return [int(c["cluster"]), int(c["narrow"]), int(c["group"][0]), int(c["group"][1]), int(c["up_group"]), plain,
            int(c["sub_down"]), int(c["tail_pack"]), int(c["down_pack"]), int(c["subtree"]), int(c["virtual"])]


def apply(engine, cfg):
    c = full(cfg)
    engine.set_cluster(c["cluster"])
    engine.set_narrow(c["narrow"])
    engine.set_group(*c["group"])
    engine.set_up_group(c["up_group"])
    engine.set_plain_up(*c["plain_up"])
    engine.set_sub_down(c["sub_down"])
    engine.set_tail_pack(c["tail_pack"])
    engine.set_down_pack(c["down_pack"])
    engine.set_nt_loads(c["nt"])
    engine.set_graph(False)
    engine.set_subtree(c["subtree"])
    engine.set_virtual(c["virtual"])


def key(tree, config):
    return f"{tree}|{config}"


def walk_tree(engine, name, tree):
    """{key: [COUNTS of every (sites, present, mode), in that order]} of one tree, every
    configuration.  Leaves the engine at the defaults, profiling off."""
    from panman_amd._lib import phase_report, phase_reset
    off, idx, root = tree
    rows = _shapes.leaf_rows(off)
    out = {key(name, cname): [] for cname, _ in CONFIGS}
    engine.set_profiling(True)
    try:
        for sites in SITES:
            codes, cons = _shapes.mixed_columns(np.random.default_rng(sites), off, idx, root, sites)
            for present in PRESENT:
                mask = None
                if not present:
                    mask = np.ones(codes.shape, bool)
                    mask[0, 0] = False
                for cname, cfg in CONFIGS:
                    apply(engine, cfg)
                    engine.tree_upload(off, idx, root)
                    engine.leaves_upload(codes, rows, mask)
                    engine.sites_upload(cons)
                    for mode in MODES:
                        engine.kernel_times(6)   # (reading the spans empties them)
                        phase_reset()
                        engine.run(mode)
                        _, launches = engine.kernel_times(6)
                        ph = dict(phase_report())
                        out[key(name, cname)].append([int(launches[k]) for k in TIMER_CLASSES] +
                                                     [int(ph.get(p, -1)) for p in PHASES])
    finally:
        engine.set_profiling(False)
        apply(engine, {})
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)["entries"]


def write_golden(entries):
    with open(GOLDEN, "w") as f:
        f.write('{"counts": ' + json.dumps(list(COUNTS)) + ',\n "entries": {\n')
        f.write(",\n".join(f'  {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in entries.items()))
        f.write("\n }}\n")


__all__ = ["CONFIGS", "COUNTS", "MODES", "PRESENT", "SITES", "apply", "key", "load_golden", "option_values", "tree_set",
           "walk_tree", "write_golden"]
