"""Inputs of pick_pair's recorded reference runs (tests/golden/make_golden_pair.py) and of the tests that replay them: made from
fixed seeds, never stored -- the manifest holds their SHA-256.  CASES names, per recorded run, the two inputs, the command line
and the ROUTE that pair_ref's certificate predicts for the tool (identity, join, or host: the walk itself).  The prediction is
written down here and held to pair_ref by tests/test_pair_golden.py; the GPU tests hold the tool and the ABI to it."""
import hashlib
import os

import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
FASTQ = ["allzero.fq", "badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "crlf.fq", "empty.fq", "len0.fq", "longname.fq", "multi.fq.gz",
         "nonl.fq", "short.fq", "stale.fq", "syn_100.fq.gz", "syn_var_a.fq", "syn_var_b.fq.gz", "t.fq", "t.fq.gz", "trunc.fq"]   # make_golden_uniq.py's list
OWN = "pair/inputs/"
BORDERS = (15, 16, 17, 31, 32, 33)      # offsets of the first space next to the 16-byte loads' borders


def fq(recs):
    return b"".join(b"%s\n%s\n+\n%s\n" % r for r in recs)


def body(rs, n):
    return bytes(rs.choice(ACGT, n)), bytes(rs.randint(33, 74, n).astype(np.uint8))


def name_of(k, mate, width=None):
    """An Illumina-style name, ascending with k as bytes; width: pad the part in front of the space to that many bytes."""
    head = b"@SIM:7:FC1:%d:%04d:%05d" % (1 + k // 100000000, k // 10000 % 10000, k % 10000 * 3 + 11)
    if width is not None:
        head = b"@" + b"P" * (width - 10) + b"%09d" % k
    return head + b" %d:N:0:ATCACG" % mate


def mates(seed, keys_a, keys_b, length=36, width=None, name=name_of):
    """Two files over the key lists: the records of one key are mates."""
    rs = np.random.RandomState(seed)

    def one(keys, mate, n):
        seq, qual = rs.choice(ACGT, (len(keys), n)), rs.randint(33, 74, (len(keys), n)).astype(np.uint8)
        return fq([(name(k, mate, width), seq[i].tobytes(), qual[i].tobytes()) for i, k in enumerate(keys)])

    return one(keys_a, 1, length), one(keys_b, 2, length + 1)


def named(names_a, names_b, seed=5):
    rs = np.random.RandomState(seed)
    return fq([(n,) + body(rs, 9) for n in names_a]), fq([(n,) + body(rs, 10) for n in names_b])


def thinned(seed, n, every_a, every_b, clean=True):
    """n keys; A loses every every_a-th and B every every_b-th of them (never the last key: the walk must end on a pair).  clean:
    B keeps a key whose predecessor A has lost -- a B-only record directly in front of an A-only one makes the walk pair that
    A-only record with the NEXT B record (the mispair), and no proposal verifies."""
    rs = np.random.RandomState(seed)
    keys = np.sort(rs.choice(10 * n, n, replace=False))
    lost_a = lambda i: i % every_a == 1 and i != n - 1
    lost_b = lambda i: i % every_b == 2 and i != n - 1 and not (clean and (lost_a(i) or lost_a(i - 1)))
    return [int(k) for i, k in enumerate(keys) if not lost_a(i)], [int(k) for i, k in enumerate(keys) if not lost_b(i)]


def own_inputs():
    """{name: bytes}; a pair of inputs is NAME_a.fq and NAME_b.fq."""
    f = {}

    def put(name, ab):
        f[name + "_a.fq"], f[name + "_b.fq"] = ab

    # ---- the quirks of the walk
    put("mispair", named([b"@b 1", b"@e 1"], [b"@a 2", b"@c 2", b"@e 2"]))
    put("prefix", named([b"@r1 1", b"@r2 1"], [b"@r10 2", b"@r2 2"]))
    put("prefix_gap", named([b"@r1 1", b"@r3 1"], [b"@r10 2", b"@r2 2", b"@r3 2"]))
    put("nospace_same", named([b"@q1", b"@q2", b"@q3"], [b"@q1", b"@q2", b"@q3"]))
    put("nospace_longer_b", named([b"@q1", b"@q2"], [b"@q1/2", b"@q2/2"]))
    put("nospace_gap", named([b"@q1", b"@q3"], [b"@q1", b"@q2", b"@q3"]))
    put("nospace_in_b", named([b"@q1 1", b"@q2 1"], [b"@q1", b"@q2"]))
    put("unsorted_all_paired", named([b"@z 1", b"@a 1", b"@m 1", b"@b 1"], [b"@z 2", b"@a 2", b"@m 2", b"@b 2"]))
    put("unsorted_gap", named([b"@z 1", b"@a 1", b"@b 1"], [b"@z 2", b"@m 2", b"@a 2", b"@b 2"]))
    put("dups", named([b"@x 1", b"@x 1", b"@y 1"], [b"@x 2", b"@x 2", b"@y 2"]))
    put("dups_gap", named([b"@x 1", b"@x 1", b"@y 1"], [b"@w 2", b"@x 2", b"@x 2", b"@y 2"]))
    put("tail", named([b"@e 1"], [b"@a 2", b"@b 2"]))
    put("tail_b_runs_out", named([b"@a 1", b"@e 1"], [b"@a 2", b"@b 2"]))
    put("a_empty", (b"", named([], [b"@a 2"])[1]))
    put("b_empty", (named([b"@a 1"], [])[0], b""))
    put("a_runs_out", named([b"@a 1"], [b"@b 2"]))
    put("one_side_left", named([b"@a 1", b"@b 1"], [b"@a 2"]))
    put("b_left", named([b"@a 1"], [b"@a 2", b"@b 2"]))
    put("both_empty", (b"", b""))
    put("high_bytes", named([b"@\xe9a 1", b"@\xe9b 1"], [b"@\x7fz 2", b"@\xe9a 2", b"@\xe9b 2"]))
    put("b_shorter_than_k", named([b"@longname1 1", b"@longname2 1"], [b"@lo", b"@longname1 2", b"@longname2"]))
    # ---- counts, gaps, the load borders
    put("one_one", mates(11, [5], [5]))
    put("two_two", mates(12, [5, 9], [5, 9]))
    put("one_two", mates(13, [9], [5, 9]))
    put("two_one", mates(14, [5, 9], [9]))
    put("gap_start_both", mates(15, [1, 2, 7, 8, 9], [3, 4, 7, 8, 9]))
    put("gap_start_a", mates(16, [1, 2, 7, 8], [7, 8]))
    put("gap_start_b", mates(17, [7, 8], [1, 2, 7, 8]))
    put("gap_middle_both", mates(18, [1, 2, 3, 6, 7, 9], [1, 4, 5, 6, 8, 9]))
    put("thinned_300", mates(19, *thinned(19, 300, 7, 11)))
    put("thinned_70_var", mates(20, *thinned(20, 70, 5, 3), length=150))
    put("thinned_mispairs", mates(23, *thinned(23, 60, 5, 3, clean=False)))
    for w in BORDERS:
        put("space_at_%d" % w, mates(30 + w, [1, 2, 4, 5, 6], [1, 3, 4, 6], width=w))
        put("space_at_%d_same" % w, mates(60 + w, [3, 1, 2], [3, 1, 2], width=w))
    a, b = mates(21, [1, 2, 4, 5], [1, 3, 4, 5])
    put("crlf", (a.replace(b"\n", b"\r\n"), b.replace(b"\n", b"\r\n")))
    put("nonl_both", (a[:-1], b[:-1]))
    put("nonl_a", (a[:-1], b))
    put("lone_line", (a + b"@lonely", b))
    put("trunc_b", (a, b[:-40]))
    a, b = mates(22, [1, 2, 3], [1, 2, 3])
    put("same3", (a, b))
    return f


# id, inputs (a name of tests/golden/fastq/ or OWN + name), the route predicted; args: None = -1 a -2 b -o o
def _case(cid, a, b, route, args=None):
    return {"id": cid, "a": a, "b": b, "route": route, "args": args}


def cases():
    c = []
    own = lambda n: (OWN + n + "_a.fq", OWN + n + "_b.fq")
    host = ("mispair", "unsorted_gap", "dups_gap", "tail", "tail_b_runs_out", "a_empty", "b_empty", "a_runs_out", "one_side_left", "b_left",
            "nospace_longer_b", "thinned_mispairs", "trunc_b")
    identity = ("prefix", "nospace_same", "nospace_in_b", "unsorted_all_paired", "dups", "both_empty", "one_one", "two_two", "same3") + \
        tuple("space_at_%d_same" % w for w in BORDERS)
    names = sorted({n[:-5] for n in own_inputs()})
    for n in names:
        c.append(_case(n, *own(n), route="host" if n in host else "identity" if n in identity else "join"))
    irregular = ("badcrc.fq.gz", "badcrc_mid.fq.gz", "badisize.fq.gz", "longname.fq", "trunc.fq")
    for f in FASTQ:
        c.append(_case("self_" + f.replace(".", "_"), "fastq/" + f, "fastq/" + f, "host" if f in irregular else "identity"))
    c.append(_case("o_before_1", *own("same3"), route="identity", args=["-o", "o", "-1", "{a}", "-2", "{b}"]))
    c.append(_case("only_1_and_2", *own("thinned_300"), route="join", args=["-1", "{a}", "-2", "{b}"]))
    c.append(_case("o_twice", *own("same3"), route="identity", args=["-o", "x", "-1", "{a}", "-o", "y", "-2", "{b}", "-o", "z"]))
    c.append(_case("gz_inputs", "fastq/syn_100.fq.gz", "fastq/syn_100.fq.gz", "identity", args=["-2", "{b}", "-1", "{a}", "-o", "o"]))
    c.append(_case("missing_1", None, OWN + "same3_b.fq", None, args=["-1", "no_such_file.fq", "-2", "{b}", "-o", "o"]))
    c.append(_case("missing_2", OWN + "same3_a.fq", None, None, args=["-1", "{a}", "-2", "no_such_file.fq", "-o", "o"]))
    c.append(_case("no_arguments", None, None, None, args=[]))
    c.append(_case("help", None, None, None, args=["-h"]))
    c.append(_case("unknown_option", None, None, None, args=["-x"]))
    return c


# ---- inputs of the GPU tests that are not recorded (checked against pair_ref) --------------------------------------------

def big_gap(n=5000):
    """A gap of n consecutive B-only records: the join's guess lies far away and the ranks cross the scan's tiles."""
    return mates(41, list(range(0, 40)) + list(range(40 + n, 90 + n)), list(range(0, 90 + n)))


def large(n=100000):
    return mates(42, *thinned(42, n, 50, 47), length=20)


def digest(data):
    return hashlib.sha256(data).hexdigest()


def materialize(directory, digests=None):
    """Writes every input into `directory`; with `digests` ({name: sha256}) checks each one first."""
    files = own_inputs()
    if digests is not None:
        assert sorted(files) == sorted(digests), sorted(set(files) ^ set(digests))
    for name, data in files.items():
        if digests is not None:
            assert digest(data) == digests[name], name
        with open(os.path.join(directory, name), "wb") as fh:
            fh.write(data)
    return {name: digest(data) for name, data in files.items()}
