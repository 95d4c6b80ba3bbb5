"""pick_pair.c restated: the framing (four gzgets lines of at most 1023 bytes, gzeof tested behind the first), the walk of the two
files against each other, and -- as plain loops -- the propose-and-verify procedure that the device runs instead of the walk
(docs/kernels/fastq_pair.md).  No GPU, no library of the project."""

LINE = 1023          # gzgets(file, buf, 1024)
NONE = None


class NoAnswer(Exception):
    """The reference dereferences a NULL record (or a NULL line) there: SIGSEGV."""


class Lines:
    """zlib's gzgets / gzeof over a whole inflated stream (csrc/host/mem_lines.hpp)."""

    def __init__(self, data):
        self.d, self.pos, self.past = data, 0, False

    def gets(self):
        d, pos = self.d, self.pos
        if pos >= len(d):
            self.past = True
            return None
        room = min(len(d) - pos, LINE)
        nl = d.find(b"\n", pos, pos + room)
        k = nl - pos + 1 if nl >= 0 else room
        if nl < 0 and pos + k == len(d) and k < LINE:
            self.past = True
        self.pos = pos + k
        return d[pos:pos + k]


def cstr(line):
    """What strlen / strdup see of a buffer."""
    z = line.find(b"\0")
    return line if z < 0 else line[:z]


def next_record(lines):
    """readNextNode: (name, sequence, quality line) or None."""
    line = lines.gets()
    if lines.past:
        return None

    def chopped(x):
        if x is None:
            raise NoAnswer("strlen(NULL)")
        x = cstr(x)
        if not x:
            raise NoAnswer("buf[-1] = 0")
        return x[:-1]

    name = chopped(line)
    seq = chopped(lines.gets())
    lines.gets()
    qual = lines.gets()
    if qual is None:
        raise NoAnswer("strdup(NULL)")
    return name, seq, cstr(qual)


def records(data):
    """Every record of a stream (the walk reads each file front to back whatever the other holds)."""
    lines, out = Lines(data), []
    while True:
        r = next_record(lines)
        if r is None:
            return out
        out.append(r)


def regular(data):
    """The text the device frames: no NUL byte, no line of 1023 or more bytes, whole records (a last line may lack its newline; one
    more line without a newline behind the last record is no record)."""
    if b"\0" in data:
        return False
    lines = data.split(b"\n")
    open_end = lines[-1] != b""
    if not open_end:
        lines.pop()
    if any(len(x) + 1 > LINE for x in lines):      # (the line and its newline: gzgets would split it)
        return False
    n = len(lines)
    return n % 4 == 0 or (open_end and n % 4 == 1)


def klen(name):
    k = name.find(b" ")
    return None if k < 0 else k


def compare(a_name, b_name):
    """The sign of strncmp(a, b, strchr(a, ' ') - a): unsigned bytes, both names end in NUL, and without a space the count is
    (size_t)(NULL - a) -- everything."""
    k = klen(a_name)
    x, y = a_name + b"\0", b_name + b"\0"
    if k is not None:
        x, y = x[:k], y[:k]
    for p in range(min(len(x), len(y))):
        if x[p] != y[p]:
            return -1 if x[p] < y[p] else 1
        if x[p] == 0:
            return 0
    return 0      # (k bytes agree; both hold k bytes or the shorter one ended in its NUL above)


def text_of(r):
    return r[0] + b"\n" + r[1] + b"\n+\n" + r[2]


def walk(data_a, data_b):
    """load_fastq_file's loop.  Returns the partition ([paired A ordinals or None per A], the same for B) -- as lists pe_a, se_a,
    pe_b, se_b of ordinals -- or raises NoAnswer where the reference crashes."""
    la, lb = Lines(data_a), Lines(data_b)
    ia = ib = -1
    pe_a, se_a, pe_b, se_b = [], [], [], []

    def nxt(lines, i):
        r = next_record(lines)
        return r, i + 1

    while True:
        a, ia = nxt(la, ia)
        b, ib = nxt(lb, ib)
        while a is not None:
            if b is None:
                raise NoAnswer("line2 is NULL")
            if compare(a[0], b[0]) >= 0:
                break
            se_a.append(ia)
            a, ia = nxt(la, ia)
        while b is not None:
            if a is None:
                raise NoAnswer("line1 is NULL")
            if compare(a[0], b[0]) <= 0:
                break
            se_b.append(ib)
            b, ib = nxt(lb, ib)
        if a is None and b is None:
            return pe_a, se_a, pe_b, se_b
        if a is not None:
            pe_a.append(ia)
        if b is not None:
            pe_b.append(ib)


def outputs(data_a, data_b, part):
    """The four inflated outputs (_1_PE, _1_SE, _2_PE, _2_SE) of a partition."""
    ra, rb = records(data_a), records(data_b)
    pe_a, se_a, pe_b, se_b = part
    return [b"".join(text_of(ra[i]) for i in pe_a), b"".join(text_of(ra[i]) for i in se_a),
            b"".join(text_of(rb[j]) for j in pe_b), b"".join(text_of(rb[j]) for j in se_b)]


def run(data_a, data_b):
    """The reference's four outputs and its stderr (times masked)."""
    return outputs(data_a, data_b, walk(data_a, data_b)), "Finished load file at T s\nFinished  at T s\n"


# ---- propose and verify ----------------------------------------------------------------------------------------------

def propose_identity(names_a, names_b):
    return list(range(len(names_a))) if len(names_a) == len(names_b) else None


def propose_join(names_a, names_b):
    """Per A record the first B ordinal j with c(a, b_j) <= 0 -- found as the device finds it: outward from i * nB / nA by doubling
    steps, then by bisection, which is the first such j where B is ascending under c(a, .) -- paired where c is 0 there."""
    n_a, n_b = len(names_a), len(names_b)
    m = []
    for i, a in enumerate(names_a):
        lo, hi, eq = -1, n_b, False
        if n_b:
            probe, direction, gallop, step = min(i * n_b // n_a, n_b - 1), 0, True, 1
            while True:
                c = compare(a, names_b[probe])
                p = c <= 0
                if p:
                    hi, eq = probe, c == 0
                else:
                    lo = probe
                if direction == 0:
                    direction = -1 if p else 1
                elif gallop and (direction < 0) != p:
                    gallop = False
                if hi - lo <= 1:
                    break
                nxt = lo + (hi - lo) // 2
                if gallop:
                    cand = hi - step if direction < 0 else lo + step
                    step <<= 1
                    if lo < cand < hi:
                        nxt = cand
                    else:
                        gallop = False
                probe = nxt
        m.append(hi if hi < n_b and eq else NONE)
    return m


def certify(names_a, names_b, m):
    """V1 .. V5 over a proposal m (per A record a B ordinal or None).  Returns None when the proposal is what the walk produces,
    else the smallest failing (mate, ordinal)."""
    n_a, n_b = len(names_a), len(names_b)
    pairs = [(i, j) for i, j in enumerate(m) if j is not NONE]
    paired_b = [False] * n_b
    for _, j in pairs:
        paired_b[j] = True
    fails = []
    rank = 0                                # pairs in front of A record i
    for i in range(n_a):
        if m[i] is not NONE:
            j = m[i]
            if rank and pairs[rank - 1][1] >= j:
                fails.append((0, i))        # V1
            elif compare(names_a[i], names_b[j]) != 0:
                fails.append((0, i))        # V2
            rank += 1
        elif rank >= len(pairs):
            fails.append((0, i))            # V5
        else:
            first = pairs[rank - 1][1] + 1 if rank else 0
            if first >= n_b or compare(names_a[i], names_b[first]) >= 0:
                fails.append((0, i))        # V3
    rank = 0                                # paired B records in front of B record j
    for j in range(n_b):
        if paired_b[j]:
            rank += 1
        elif rank >= len(pairs):
            fails.append((1, j))            # V5
        elif compare(names_a[pairs[rank][0]], names_b[j]) <= 0:
            fails.append((1, j))            # V4
    return min(fails) if fails else None


def partition_of(m, n_b):
    paired = {j for j in m if j is not NONE}
    return ([i for i, j in enumerate(m) if j is not NONE], [i for i, j in enumerate(m) if j is NONE],
            [j for j in range(n_b) if j in paired], [j for j in range(n_b) if j not in paired])


def device(data_a, data_b):
    """What the session answers for two REGULAR streams: (route, partition) with route "identity" or "join", or ("host", fail)
    where neither proposal verifies."""
    names_a, names_b = [r[0] for r in records(data_a)], [r[0] for r in records(data_b)]
    if not names_a and not names_b:
        return "identity", ([], [], [], [])
    fail = None
    for route, propose in (("identity", propose_identity), ("join", propose_join)):
        m = propose(names_a, names_b)
        if m is None:
            continue
        fail = certify(names_a, names_b, m)
        if fail is None:
            return route, partition_of(m, len(names_b))
    return "host", fail


def predicted_route(data_a, data_b):
    """The route the tool takes for two input files' inflated bytes."""
    if not (regular(data_a) and regular(data_b)):
        return "host"
    return device(data_a, data_b)[0]
