"""The two-wave form of the hot V1 merge kernel (ym_fast.hip k_fast_merge_v1_split: wave 0 the struct half,
wave 1 the delete-set half of one document): hand-encoded documents at the boundaries of its schedule, declines
raised by one half only, and agreement with the one-wave kernel (YMERGE_FAST_SPLIT=0).  Every case runs
device-resident through ym_merge and ym_merge_async, with u32 and u64 update offsets, against the oracle.

Run as a script (`python tests/test_gpu_fast_split.py OUT`) it merges the same batches and pickles what it
got into OUT: the test that compares the two kernels starts it once per YMERGE_FAST_SPLIT value, since the
library reads the variable once per process."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

IN_HOT = 2432  # ym_fast.hip: the hot pass's document byte limit
YM_ERR_CAPACITY = 9


# ---- hand-encoded V1 updates ------------------------------------------------------------------------------
def _vu(v):
    out = bytearray()
    while v > 127:
        out.append(0x80 | (v & 127))
        v >>= 7
    out.append(v)
    return bytes(out)


def _ds_bytes(ranges):
    """The delete set {client: [(clock, len), ...]} (DeleteSet.js:219-232)."""
    b = bytearray(_vu(len(ranges)))
    for client, rs in ranges.items():
        b += _vu(client) + _vu(len(rs))
        for clock, ln in rs:
            b += _vu(clock) + _vu(ln)
    return bytes(b)


def _ds_update(ranges):
    """A V1 update with no structs and the delete set `ranges`."""
    return b"\x00" + _ds_bytes(ranges)


def _text_update(client, clock, s, ds=b"\x00"):
    """A V1 update inserting the ASCII bytes `s` as one ContentString (client, clock, no origin, parent ykey
    "t"), followed by the encoded delete set `ds` (default: empty)."""
    return _vu(1) + _vu(1) + _vu(client) + _vu(clock) + bytes([0x04, 1, 1, ord("t")]) + _vu(len(s)) + s + ds


CLIENTS = [5, 300, 2**31 + 7]


def _ranges(rng, n):
    clocks = sorted(int(c) for c in rng.choice(400, size=n, replace=False))
    return [(c, int(rng.integers(1, 6))) for c in clocks]


def _doc(rng, n1, n2, ranges_per=1, struct_ds=False, shuffle=True, max_ranges=None):
    """n1 updates with one client section each (three clients, clocks ascending per client with a few gaps) and
    n2 delete-only updates of `ranges_per` ranges; struct_ds: half of the updates with structs carry a delete
    set of one range too (at most max_ranges ranges in all, when given).  shuffle: the updates in random order
    (else in clock order per client)."""
    nxt = {c: 0 for c in CLIENTS}
    ups = []
    left = (max_ranges if max_ranges is not None else 1 << 30) - n2 * ranges_per
    for _ in range(n1):
        c = CLIENTS[int(rng.integers(0, len(CLIENTS)))]
        s = bytes(int(x) for x in rng.integers(97, 123, size=int(rng.integers(1, 4))))
        clock = nxt[c] + (int(rng.integers(1, 4)) if rng.random() < 0.15 else 0)
        nxt[c] = clock + len(s)
        ds = b"\x00"
        if struct_ds and rng.random() < 0.5 and left > 0:
            left -= 1
            ds = _ds_bytes({CLIENTS[int(rng.integers(0, len(CLIENTS)))]: _ranges(rng, 1)})
        ups.append(_text_update(c, clock, s, ds))
    for _ in range(n2):
        ups.append(_ds_update({CLIENTS[int(rng.integers(0, len(CLIENTS)))]: _ranges(rng, ranges_per)}))
    if shuffle:
        ups = [ups[int(i)] for i in rng.permutation(len(ups))]
    assert sum(len(u) for u in ups) <= IN_HOT, (n1, n2, sum(len(u) for u in ups))
    return ups


N1 = [1, 2, 63, 64, 65, 76, 100, 127]
N2 = [0, 1, 39, 64]
PER_CASE = 6


def _boundary_docs():
    """(n1, n2) at every boundary of the schedule with k <= 128; no delete ranges at all where n2 == 0."""
    rng = np.random.default_rng(707)
    docs, general = [], 0
    for n1 in N1:
        for n2 in N2:
            if n1 + n2 > 128:
                continue
            for i in range(PER_CASE):
                docs.append(_doc(rng, n1, n2, shuffle=i % 2 == 1))
                general += n1 + n2 <= 1  # (a single update is not the LDS kernels' shape)
    return docs, general


def _struct_ds_docs():
    """Updates with structs that carry non-empty delete sets (wave 1's round after barrier A), alone and mixed
    with delete-only updates; more than 64 sections and more than 64 delete ranges (two records per lane)."""
    rng = np.random.default_rng(708)
    docs = []
    for n1, n2, rp, sds in [(2, 0, 1, True), (64, 0, 1, True), (65, 0, 1, True), (100, 0, 1, True), (2, 39, 1, True),
                            (63, 64, 1, True), (76, 39, 1, True), (2, 39, 3, False), (65, 39, 3, False), (76, 30, 3, True),
                            (64, 21, 3, True), (20, 64, 2, False)]:
        for i in range(PER_CASE):
            docs.append(_doc(rng, n1, n2, ranges_per=rp, struct_ds=sds, shuffle=i % 2 == 1, max_ranges=128))
    return docs, 0


def _pad_to(ups, total):
    """ups plus one update whose text brings the document to exactly `total` bytes."""
    have = sum(len(u) for u in ups)
    for n in range(130, 2440):  # (a two-byte length: one candidate per size)
        u = _text_update(77, 0, b"x" * n)
        if have + len(u) == total:
            return ups + [u]
    raise AssertionError((have, total))


def _limit_docs():
    """Documents of exactly the hot pass's byte limit (hot kernel) and one byte over (its retry pass)."""
    rng = np.random.default_rng(709)
    docs = []
    for i in range(16):
        base = _doc(rng, int(rng.integers(2, 70)), int(rng.integers(0, 40)), struct_ds=i % 2 == 0)
        docs.append(_pad_to(base, IN_HOT))
        docs.append(_pad_to(base, IN_HOT + 1))
        docs.append(_pad_to(base, IN_HOT - 1))
    return docs, 0


def _decline_docs():
    """Documents only one half of the kernel declines, among plain ones; every second document is plain."""
    rng = np.random.default_rng(710)
    docs, general = [], 0
    gc = _vu(1) + _vu(1) + _vu(9) + _vu(0) + bytes([0]) + _vu(3) + b"\x00"        # one GC struct of length 3
    skip = _vu(1) + _vu(1) + _vu(9) + _vu(0) + bytes([10]) + _vu(3) + b"\x00"     # one Skip of length 3
    trunc_item = _vu(1) + _vu(1) + _vu(9) + _vu(0) + bytes([0x04, 1, 1, ord("t"), 5, ord("a")])  # string cut short
    for i in range(PER_CASE):
        n1 = [2, 40, 64, 70][i % 4]
        plain = _doc(rng, n1, 20, struct_ds=i % 2 == 0)
        bad = [
            plain + [gc],                                         # wave 0 (or wave 1's share when n1 >= 64)
            [skip] + plain,
            plain + [b"\x00" + _vu(1) + _vu(5) + _vu(2) + _vu(1) + _vu(1)],          # delete set cut short (wave 1)
            plain + [b"\x00" + _vu(1) + _vu(5)],                                     # ... inside its header
            plain + [b"\x00"],                                                       # ... missing altogether
            _doc(rng, 2, 64, ranges_per=3),                                          # 192 ranges > 128 (wave 1)
            _doc(rng, 70, 20) + [trunc_item],                                        # malformed, in wave 1's W1 share
            _doc(rng, 64, 20) + [trunc_item],                                        # ... the 65th
            _doc(rng, 63, 20) + [trunc_item],                                        # ... the 64th: wave 0's last lane
            _doc(rng, 76, 10) + [_text_update(9, 0, b"ab")[:-1]],                    # struct update without a delete set
        ]
        for b in bad:
            docs.append(b)
            docs.append(_doc(rng, n1, 20))
    return docs, None


def _overlong_docs():
    """Delete sets followed by bytes their counts do not cover (yjs stops reading at the counts), and with counts
    that promise more than the update holds: whichever path takes them, the oracle's bytes or error."""
    rng = np.random.default_rng(712)
    docs = []
    for i in range(PER_CASE):
        plain = _doc(rng, [2, 40, 64, 70][i % 4], 20, struct_ds=i % 2 == 0)
        docs.append(plain + [_ds_update({5: _ranges(rng, 1)}) + b"\x07\x07"])
        docs.append(plain + [_text_update(9, 0, b"ab", _ds_bytes({5: _ranges(rng, 2)}) + b"\x01")])
        docs.append(plain + [b"\x00" + _vu(2) + _vu(5) + _vu(1) + _vu(1) + _vu(1)])
    return docs, None


BATCHES = {"boundary": _boundary_docs, "struct_ds": _struct_ds_docs, "limit": _limit_docs, "decline": _decline_docs,
           "overlong": _overlong_docs}


def _capacity_case():
    """Two documents; the second has a struct section and a delete set of several bytes.  Returns the packed batch
    and the arena sizes that end at given offsets into the second document's slot."""
    from yjs_amd import pack_docs
    rng = np.random.default_rng(711)
    first = _doc(rng, 10, 5)
    structs = [u for u in _doc(rng, 30, 0)]
    dels = [_ds_update({CLIENTS[i % 3]: _ranges(rng, 2)}) for i in range(8)]
    a, o, d = pack_docs([first, structs + dels])
    slot = 2 * (int(o[int(d[1])]) - int(o[0])) + 64 * 1
    return (a, o, d), structs, (slot + 63) & ~63


# ---- running a batch on the device ------------------------------------------------------------------------
def _dev(torch, arena, upd_off, doc_upd, cap, off32):
    g = dict(arena=torch.from_numpy(np.array(arena, np.uint8)).cuda(),
             off=torch.from_numpy(upd_off.astype(np.uint32).view(np.int32) if off32 else upd_off.astype(np.uint64).view(np.int64)).cuda(),
             doc=torch.from_numpy(doc_upd.astype(np.uint32).view(np.int32)).cuda())
    nd = len(doc_upd) - 1
    g.update(out=torch.zeros(cap, dtype=torch.uint8, device="cuda"), oo=torch.zeros(nd, dtype=torch.int64, device="cuda"),
             ol=torch.zeros(nd, dtype=torch.int64, device="cuda"), st=torch.full((nd,), -1, dtype=torch.int32, device="cuda"))
    return g


def _outputs(g):
    a, oo, ol, st = g["out"].cpu().numpy(), g["oo"].cpu().numpy(), g["ol"].cpu().numpy(), g["st"].cpu().numpy()
    return [a[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() if st[i] == 0 else int(st[i]) & 0xff for i in range(len(st))]


def _run_sync(engine, a, o, d, off32):
    import torch
    g = _dev(torch, a, o, d, 4 * len(a) + 128 * (len(d) - 1) + 8192, off32)
    rc, _ = engine.run_device("merge", 1, g["arena"], g["off"], g["doc"], g["out"], g["oo"], g["ol"], g["st"])
    assert rc == 0, rc
    torch.cuda.synchronize()
    return _outputs(g), {k: engine.stats[k] for k in ("docs", "docs_fast", "docs_general", "docs_error", "bytes_out")}


def _run_async(engine, a, o, d, off32, cap=None):
    import torch
    g = _dev(torch, a, o, d, cap if cap is not None else 2 * int(o[-1]) + 64 * (len(d) - 1) + 64, off32)
    pend = torch.zeros(1, dtype=torch.int32, device="cuda")
    call = engine.prepare_merge_async(1, g["arena"], g["off"], g["doc"], g["out"], g["oo"], g["ol"], g["st"], pending=pend)
    assert call() == 0
    torch.cuda.synchronize()
    return _outputs(g), int(pend.item())


@pytest.fixture(scope="module")
def engine():
    from yjs_amd import Engine
    return Engine(0)


@pytest.fixture(scope="module")
def batches():
    """name -> (packed batch, the oracle's outputs (bytes, or the status of yjs's error), expected general-path
    documents or None): computed once, read-only."""
    import oracle_ref as O
    from yjs_amd import pack_docs
    out = {}
    for name, make in BATCHES.items():
        docs, general = make()
        a, o, d = pack_docs(docs)
        outs, status, _ = O.batch("merge", 1, a, o, d, nthreads=8)
        want = [outs[i] if status[i] == 0 else int(status[i]) for i in range(len(docs))]
        out[name] = ((a, o, d), want, general)
    return out


@pytest.mark.parametrize("off32", [True, False], ids=["u32", "u64"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_split_schedule_matches_oracle(engine, batches, name, off32):
    from yjs_amd.engine import YM_PENDING
    (a, o, d), want, general = batches[name]
    nd = len(want)
    got, stats = _run_sync(engine, a, o, d, off32)
    bad = [i for i in range(nd) if got[i] != want[i]]
    assert not bad, (name, bad[:10])
    agot, pend = _run_async(engine, a, o, d, off32)
    bad = [i for i in range(nd) if agot[i] != want[i] and agot[i] != YM_PENDING]
    assert not bad, (name, bad[:10])
    npend = sum(1 for x in agot if x == YM_PENDING)
    assert npend == pend
    print(name, "docs", nd, "general", stats["docs_general"], "fast", stats["docs_fast"], "async pending", pend)
    if name == "decline":
        # every damaged document (the even ones) leaves the LDS kernels, every plain one stays
        assert all((agot[i] == YM_PENDING) == (i % 2 == 0) for i in range(nd)), [i for i in range(nd) if (agot[i] == YM_PENDING) != (i % 2 == 0)][:10]
        # (docs_fast counts the LDS kernels' documents; the others go to the general path or, by their shape, to
        # the large-document pipeline first)
        assert stats["docs_fast"] == nd // 2 and 0 < stats["docs_general"] <= nd // 2, stats
    elif name == "limit":
        # one byte over the limit: declined by the hot kernel (async), taken by its retry pass (sync)
        over = [i for i in range(nd) if i % 3 == 1]
        assert [i for i in range(nd) if agot[i] == YM_PENDING] == over
        assert stats["docs_general"] == 0 and stats["docs_fast"] == nd, stats
    elif general is not None:
        assert pend == general and stats["docs_general"] == general and stats["docs_fast"] == nd - general, stats


@pytest.mark.parametrize("off32", [True, False], ids=["u32", "u64"])
def test_split_capacity_per_half(engine, off32):
    """An output arena that ends inside the second document's slot: before the end of its struct section (wave
    0's check) and after it but before the end of its delete set (wave 1's check) the document reports
    YM_ERR_CAPACITY; an arena that ends exactly at its last byte holds it; the first document is intact."""
    import oracle_ref as O
    from yjs_amd import pack_docs
    (a, o, d), structs, slot_al = _capacity_case()
    outs, status, _ = O.batch("merge", 1, a, o, d)
    assert (status == 0).all()
    sa, so, sd = pack_docs([structs])
    souts, sst, _ = O.batch("merge", 1, sa, so, sd)
    assert sst[0] == 0 and souts[0][-1] == 0
    struct_len, total = len(souts[0]) - 1, len(outs[1])  # the struct section; with the delete set
    assert outs[1][:struct_len] == souts[0][:-1] and total >= struct_len + 4
    for cap, want1 in [(slot_al + struct_len - 1, YM_ERR_CAPACITY), (slot_al + 1, YM_ERR_CAPACITY),
                       (slot_al + struct_len, YM_ERR_CAPACITY), (slot_al + struct_len + 2, YM_ERR_CAPACITY),
                       (slot_al + total - 1, YM_ERR_CAPACITY), (slot_al + total, outs[1])]:
        got, pend = _run_async(engine, a, o, d, off32, cap=cap)
        assert got[0] == outs[0] and got[1] == want1 and pend == 0, (cap - slot_al, struct_len, total, got[1], pend)


def _child_results():
    """What this process's library gives for every batch (the script form)."""
    from yjs_amd import Engine, pack_docs
    engine = Engine(0)
    res = {}
    for name, make in BATCHES.items():
        docs, _ = make()
        a, o, d = pack_docs(docs)
        for off32 in (True, False):
            res[name, "sync", off32] = _run_sync(engine, a, o, d, off32)
            res[name, "async", off32] = _run_async(engine, a, o, d, off32)
    (a, o, d), structs, slot_al = _capacity_case()
    for extra in range(0, 400, 7):
        res["capacity", extra] = _run_async(engine, a, o, d, True, cap=slot_al + extra)
    return res


def test_split_agrees_with_one_wave_kernel(tmp_path):
    """The same batches under YMERGE_FAST_SPLIT=0 and =1, each in a fresh process: identical outputs, statuses,
    pending counts and path statistics (declines and ST_CAPACITY included)."""
    res = {}
    for split in ("0", "1"):
        out = str(tmp_path / f"split{split}.pkl")
        env = dict(os.environ, YMERGE_FAST_SPLIT=split)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(out, "rb") as f:
            res[split] = pickle.load(f)
    assert res["0"].keys() == res["1"].keys()
    for key in res["0"]:
        r0, r1 = res["0"][key], res["1"][key]
        assert r0 == r1, key


if __name__ == "__main__":
    with open(sys.argv[1], "wb") as f:
        pickle.dump(_child_results(), f)
