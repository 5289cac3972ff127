"""The oracle's side of the size ladder (tools/size_ladder.py), shared by tests/test_size_ladder_cpu.py and
tests/test_gpu_size_ladder.py: per rung its code and batch, per symbol length the codewords and received symbols, per
(max_sweeps, do_ml) every expected byte and word.  Computed once per process, read-only; the expectation is always made from the
flags normalised to 0 / 1."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import size_ladder as sl  # noqa: E402

Want = namedtuple("Want", "out sweeps residual status erased_out residual_src")
_CACHE = {}


def rung_case(name):
    """dict: rung, code, planted, batch, facts, oc (OracleCode)"""
    if name not in _CACHE:
        from oracle import oracle_py
        rung = sl.BY_NAME[name]
        code, planted = sl.ladder_code(rung)
        b = sl.batch(rung, code, planted)
        b.flags.setflags(write=False)
        _CACHE[name] = dict(rung=rung, code=code, planted=planted, batch=b, facts=sl.code_facts(code), oc=oracle_py.OracleCode(code))
    return _CACHE[name]


def symbols(name, S):
    """dict: src [F, k, S], cw [F, n, S] (the oracle's encoder), sym [F, n, S] (received)"""
    key = (name, S)
    if key not in _CACHE:
        c = rung_case(name)
        F = len(c["batch"].kinds)
        src = sl.source(c["rung"], S, F)
        cw = np.stack([c["oc"].encode(src[f]).reshape(c["code"].n, S) for f in range(F)])
        sym = sl.received(cw, c["batch"])
        for a in (src, cw, sym):
            a.setflags(write=False)
        _CACHE[key] = dict(src=src, cw=cw, sym=sym, F=F)
    return _CACHE[key]


def status_of(info, rc):
    """the library's status word from the oracle's info / return code (tests/test_gpu_fuzz.py)"""
    return 0 if info[0] == 0 else (3 if (rc == -2 or not info[1]) else (2 if info[2] else 1))


def want(name, S, max_sweeps, do_ml):
    """Want(...) of the batch.  A status-3 frame keeps its received symbols and holds the symbols the sweeps solved: that is the
    oracle's output with the ML stage off.  erased_out is the sweeps' mask for status 2 / 3, zero otherwise."""
    key = (name, S, max_sweeps, do_ml)
    if key not in _CACHE:
        c, s = rung_case(name), symbols(name, S)
        oc, fl, n, k = c["oc"], c["batch"].flags01, c["code"].n, c["code"].k
        F = s["F"]
        out = np.zeros((F, n, S), dtype=np.uint8)
        mask = np.zeros((F, n), dtype=np.uint8)
        sw, res, st = (np.zeros(F, dtype=np.int32) for _ in range(3))
        for f in range(F):
            o, _, it, info, rc = oc.decode_packets(s["sym"][f], fl[f], itenum=max_sweeps, do_ml=do_ml)
            sw[f], res[f], st[f] = it, info[0], status_of(info, rc)
            if st[f] in (2, 3):
                o3, oe, _, _, _ = oc.decode_packets(s["sym"][f], fl[f], itenum=max_sweeps, do_ml=0)
                mask[f] = oe
                if st[f] == 3:
                    o = o3
            out[f] = o
        w = Want(out, sw, res, st, mask, mask[:, :k].sum(1).astype(np.int32))
        for a in w:
            a.setflags(write=False)
        _CACHE[key] = w
    return _CACHE[key]
