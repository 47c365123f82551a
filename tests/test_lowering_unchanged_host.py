"""lower_general and split_parts give, for every family's graphs, byte for byte what they gave before the engine's Python side
was split into per-family pieces: one digest over node lists, node arrays, pools and parts."""
import hashlib

import numpy as np

import autoscaler_specs as AS
import canary_specs as CN
import client_specs as CS
import deployer_specs as DS
import fault_specs as FS
import flow_specs as FL
import graph_family as GF
import graph_specs as GS
import health_specs as HS
import helpers as H
import link_fault_specs as LS
import mixed_specs as MX
import queue_specs as QS
import rate_limiter_specs as RS
import resilience_specs as XS
import strategy_specs as SS
from happy_simulator_amd.graph_engine import GeneralGraph, split_parts
from random_specs import graph_spec, lb_graph_spec

STRIDE = 1            # every random spec of every family (the whole set lowers in a few seconds)
# the graph family has no all_specs(): its named fixtures are the goldens, its random ones the two generators of tests/test_gpu_graph.py
GRAPH_RANDOM = 240    # ... over the k its GPU test covers with both (320 and 180)

EXTRA = ("rd_params", "cn_params")       # GraphArrays' properties that stay out of vars()


def _families():
    yield "graph", GS.build, ([H.Golden(n).spec for n in H.golden_names("graph")]
                              + [f(k) for k in range(0, GRAPH_RANDOM, STRIDE) for f in (graph_spec, lb_graph_spec)])
    for name, build, mod in (("strategy", SS.build, SS), ("rate-limiter", GF.build, RS), ("fault", GF.build, FS), ("health", GF.build, HS),
                             ("resilience", GF.build, XS), ("client", GF.build, CS), ("flow", FL.build, FL), ("mixed", MX.build, MX),
                             ("queue", QS.build, QS), ("link-fault", LS.build, LS), ("autoscaler", AS.build, AS),
                             ("deployer", DS.build, DS), ("canary", CN.build, CN)):
        n_named = len(mod.FIXTURES)
        specs = mod.all_specs()
        yield name, build, specs[:n_named] + specs[n_named::STRIDE]


def _value(v) -> bytes:
    if v is None:
        return b"-"
    if isinstance(v, bytes):
        return v
    if isinstance(v, (int, list)):                   # (as_steps / cn_params: a list per node of None or plain numbers)
        return repr(v).encode()
    return str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes()


def _arrays(h, a):
    for name in sorted(set(vars(a)) | set(EXTRA)):
        if name.startswith("_"):
            continue
        h.update(name.encode())
        h.update(_value(getattr(a, name)))


def _pools(g, table):
    ids = lambda ents: [g.node_of[id(x)] for x in ents]          # noqa: E731
    return repr(sorted((lb, (owner, ids(initial), ids(pool))) for lb, (owner, initial, pool) in table.items())).encode()


def test_every_family_lowers_to_what_the_parent_commit_lowered_it_to():
    h = hashlib.sha256()
    lowered = split = 0
    for family, build, specs in _families():
        for spec in specs:
            g = build(spec)[0].lowered()
            if not isinstance(g, GeneralGraph):
                continue
            lowered += 1
            a = g.arrays
            h.update(f"{family}/{spec.get('name', '')}".encode())
            h.update(",".join(type(x).__name__ + ":" + x.name for x in g.nodes).encode())
            _arrays(h, a)
            h.update(repr((g.n_own, sorted(g.pool_of.items()), sorted(g.dpool_of.items()), sorted(g.deploys.items()),
                           sorted(g.rr_base.items()))).encode())
            h.update(_pools(g, g.scaled))
            h.update(_pools(g, g.deployed))
            parts = split_parts(a)
            if parts is None:
                continue
            split += 1
            for ids, pos, b in parts:
                h.update(np.ascontiguousarray(ids, np.int64).tobytes())
                h.update(np.ascontiguousarray(pos, np.int64).tobytes())
                _arrays(h, b)
    assert lowered >= 1500 and split >= 100                      # (every family has graphs of the single-heap kind, several fall into parts)
    assert h.hexdigest() == "73c91a74b07d941c347832570cdfa30dfb262afda45798183ea79e5dbef091fd"
