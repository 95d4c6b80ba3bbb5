"""What `samtools view` of samtools-0.1.19 (sam_view.c, sam.c, bam.c) makes of a BAM input without regions, restated sequentially:
main_samview's options, process_aln's filters in their order, drop_rg, samopen's text header, bam_format1_core's line cut at its
first NUL, the BAM writer's cuts and zlib at the asked level.  The recorded runs of tests/golden/view/manifest.json pin it to the
compiled reference (tests/test_view_golden.py); the tool's host route (csrc/host/bam_view_host.hpp) and the device route are held
to the same recordings.

view(data, args, files) -> (stdout bytes, the -o file's bytes or None, stderr text, status); status 2 where the tool refuses.
line_length(), x31_poly() and threshold() are the closed forms the device stands on.  route(data, args) says which of the tool's
routes a run takes: 'device', 'host' (never tried) or 'abandoned' (tried, then the host route)."""
import ctypes
import math
import struct

from bai_ref import EOF_BLOCK, MSG_NO_EOF
from bamsort_ref import MSG_TRUNCATED, cut, header_bytes, member, parse

MSG_TRUNC = "[main_samview] truncated file.\n"
MSG_TARGETS = "[samopen] inconsistent number of target sequences. Output the text header.\n"
NT16 = b"=ACMGRSVTWYHKDBN"
FLAG_CHARS = b"pPuUrR12sfd"
CIGAR_STR = b"MIDNSHP=XB\0"
CIGAR_TYPE = 0x3C1A7
REFUSED_OPTS = "StTLB"
WIDTH = {"c": (1, "<b"), "C": (1, "<B"), "s": (2, "<h"), "S": (2, "<H"), "i": (4, "<i"), "I": (4, "<I")}
# the device's reasons (include/hpngs.h)
R_FLOAT, R_ANUL, R_NAME, R_AUXTYPE, R_LAYOUT, R_POS, R_RECORDS, R_TARGET, R_CIGAROP = range(1, 10)


class Undefined(Exception):
    """the reference reads memory that is not its own"""


class Refused(Exception):
    """outside the tool's scope"""


def libc_rand(seed):
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(seed & 0xffffffff))
    return libc.rand()


class Options:
    def __init__(self):
        self.count = self.bam_out = self.header = self.header_only = self.long_help = False
        self.level, self.style = -1, 0
        self.flag_on = self.flag_off = self.min_mapq = self.min_qlen = self.qual_scale = 0
        self.seed, self.frac = 0, -1.0
        self.library = self.rg = self.fn_rg = self.out = self.infile = None
        self.err = ""
        self.rest = []


def c_int(text, base=10):
    """strtol / atoi: leading blanks, a sign, the digits that are there -> (value, rest)"""
    s = text.lstrip(" \t\n")
    i = 0
    neg = False
    if s[:1] in ("+", "-"):
        neg, i = s[0] == "-", 1
    if base == 0:
        if s[i:i + 2].lower() == "0x" and s[i + 2:i + 3] in tuple("0123456789abcdefABCDEF"):
            base, i = 16, i + 2
        elif s[i:i + 1] == "0":
            base = 8
        else:
            base = 10
    digits = "0123456789abcdef"[:base]
    j = i
    while j < len(s) and s[j].lower() in digits:
        j += 1
    if j == i:
        return 0, text
    v = int(s[i:j], base)
    return (-v if neg else v), s[j:]


def c_double(text):
    """strtod of the decimal forms the tests use"""
    import re
    m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", text)
    return float(m.group(0)) if m else 0.0


def to_i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def options(args):
    """main_samview's getopt loop -> Options (rest: what follows the options)"""
    takes = set("toqfFlrTRLsQ@m")
    known = set("SbBcth1HoqfFulrxX?TRLsQ@m")
    o = Options()
    i = 0
    refused = None
    while i < len(args):
        a = args[i]
        if a == "--":
            i += 1
            break
        if not a.startswith("-") or a == "-":
            break
        j = 1
        while j < len(a):
            c = a[j]
            j += 1
            if c not in known or c == ":":
                o.err += "view: invalid option -- '%s'\n" % c
                o.long_help = True
                continue
            arg = None
            if c in takes:
                if j < len(a):
                    arg = a[j:]
                elif i + 1 < len(args):
                    i += 1
                    arg = args[i]
                else:
                    o.err += "view: option requires an argument -- '%s'\n" % c
                    o.long_help = True
                    j = len(a)
                    continue
                j = len(a)
            if c == "s":
                seed, rest = c_int(arg)
                o.seed = seed & 0xffffffff
                if o.seed:
                    o.seed = libc_rand(o.seed)
                o.frac = c_double(rest)
            elif c == "m":
                o.min_qlen = to_i32(c_int(arg)[0])
            elif c == "c":
                o.count = True
            elif c == "b":
                o.bam_out = True
            elif c == "h":
                o.header = True
            elif c == "H":
                o.header_only = True
            elif c == "o":
                o.out = arg
            elif c == "f":
                o.flag_on = to_i32(c_int(arg, 0)[0])
            elif c == "F":
                o.flag_off = to_i32(c_int(arg, 0)[0])
            elif c == "q":
                o.min_mapq = to_i32(c_int(arg)[0])
            elif c == "u":
                o.level = 0
            elif c == "1":
                o.level = 1
            elif c == "l":
                o.library = arg.encode()
            elif c == "r":
                o.rg = arg.encode()
            elif c == "R":
                o.fn_rg = arg
            elif c == "x":
                o.style = 1
            elif c == "X":
                o.style = 2
            elif c == "Q":
                o.qual_scale = to_i32(c_int(arg)[0])
            elif c == "?":
                o.long_help = True
            elif c in REFUSED_OPTS:
                refused = refused or c
        i += 1
    o.rest = args[i:]
    if o.level >= 0:
        o.bam_out = True
    if o.header_only:
        o.header = True
    o.refused = refused
    return o


# ---- a record ----

def core(r):
    tid, pos, bmq, fn, l_seq, mtid, mpos, isize = struct.unpack_from("<iiIIiiii", r, 4)
    return {"tid": tid, "pos": pos, "l_qname": bmq & 0xff, "mapq": bmq >> 8 & 0xff, "n_cigar": fn & 0xffff, "flag": fn >> 16, "l_qseq": l_seq, "mtid": mtid,
            "mpos": mpos, "isize": isize}


def layout(r):
    """(cigar, seq, qual, aux) offsets; Undefined where they lie outside the record"""
    c = core(r)
    if c["l_qseq"] < 0:
        raise Undefined("a negative sequence length")
    cg = 36 + c["l_qname"]
    sq = cg + 4 * c["n_cigar"]
    ql = sq + (c["l_qseq"] + 1) // 2
    ax = ql + c["l_qseq"]
    if ax > len(r):
        raise Undefined("a name, CIGAR, sequence or quality line runs past its record")
    return cg, sq, ql, ax


def x31(name):
    """__ac_X31_hash_string over signed chars, up to the first NUL"""
    s = name.split(b"\0")[0]
    if not s:
        return 0
    sc = lambda b: b - 256 if b >= 128 else b
    h = sc(s[0]) & 0xffffffff
    for b in s[1:]:
        h = ((h << 5) - h + sc(b)) & 0xffffffff
    return h


def x31_poly(name):
    """the device's form: the sum of s[k] * 31^(L - 1 - k) modulo 2^32, 16 lanes taking every 16th byte"""
    L = len(name)
    lanes = [0] * 16
    for k, b in enumerate(name):
        lanes[k % 16] = (lanes[k % 16] + (b - 256 if b >= 128 else b) * pow(31, L - 1 - k, 1 << 32)) & 0xffffffff
    return sum(lanes) & 0xffffffff


def threshold(frac):
    """the 24-bit integer form of -s: a record is dropped where k24 >= threshold(frac)"""
    t = math.ceil(math.ldexp(frac, 24))
    return 1 << 24 if not t < (1 << 24) else max(int(t), 0)


def aux_rg(r):
    """bam_aux_get(b, "RG"): the offset of the type byte or None"""
    _, _, _, s = layout(r)
    width = lambda t: {"C": 1, "c": 1, "A": 1, "S": 2, "s": 2, "I": 4, "i": 4, "f": 4, "F": 4}.get(t, 0)

    def at(k):
        if k >= len(r):
            raise Undefined("an aux walk leaves its record")
        return r[k]
    while s < len(r):
        k0, k1 = at(s), at(s + 1)
        s += 2
        if (k0, k1) == (82, 71):
            return s
        t = chr(at(s)).upper()
        s += 1
        if t in "ZH":
            while at(s):
                s += 1
            s += 1
        elif t == "B":
            w = width(chr(at(s)))
            if s + 5 > len(r):
                raise Undefined("an aux walk leaves its record")
            cnt, = struct.unpack_from("<i", r, s + 1)
            if cnt < 0:
                raise Undefined("an aux walk leaves its record")
            s += 5 + w * cnt
        else:
            s += width(t)
    return None


def rg_table(text):
    """sam_header2tbl(dict, "RG", "ID", "LB") of a well-formed header: the last @RG line of an ID wins"""
    tbl = {}
    for line in text.split(b"\0")[0].split(b"\n"):
        if line[:4] != b"@RG\t":
            continue
        tags = {}
        for t in line.split(b"\t")[1:]:
            tags.setdefault(t[:2], t[3:])
        if b"ID" in tags and b"LB" in tags:
            tbl[tags[b"ID"]] = tags[b"LB"]
    return tbl


def rg_messages(text):
    seen, out = set(), ""
    for line in text.split(b"\0")[0].split(b"\n"):
        if line[:4] == b"@RG\t":
            tags = {}
            for t in line.split(b"\t")[1:]:
                tags.setdefault(t[:2], t[3:])
            if b"ID" in tags and b"LB" in tags:
                if tags[b"ID"] in seen:
                    out += "[sam_header_lookup_table] They key %s not unique.\n" % tags[b"ID"].decode("latin-1")
                seen.add(tags[b"ID"])
    return out


def drop_rg(text, ids):
    t = text.split(b"\0")[0]
    out, p = b"", 0
    while True:
        q = t.find(b"\n", p)
        if q < 0:
            q = len(t)
        if q - p < 3:
            break
        toprint = False
        if t[p:p + 4] == b"@RG\t":
            r = t.find(b"\tID:", p)
            if r >= 0:
                s = r + 4
                while s < len(t) and t[s] not in (10, 9):
                    s += 1
                toprint = t[r + 4:s] in ids
        else:
            toprint = True
        if toprint:
            out += t[p:q] + b"\n"
        if q >= len(t):
            break
        p = q + 1
    return out


def scaled(r, scale):
    """-Q: every quality byte q becomes min(q * scale, 93)"""
    if scale <= 1:
        return r
    c = core(r)
    _, _, ql, ax = layout(r)
    return r[:ql] + bytes(min(q * scale, 93) for q in r[ql:ax]) + r[ax:]


def query_len(r):
    c = core(r)
    cg = 36 + c["l_qname"]
    if cg + 4 * c["n_cigar"] > len(r):
        raise Undefined("a CIGAR runs past its record")
    n = 0
    for w in struct.unpack_from("<%dI" % c["n_cigar"], r, cg):
        if (CIGAR_TYPE >> ((w & 15) << 1) & 1) or (w & 15) == 5:
            n += w >> 4
    return to_i32(n)


def drops(o, r, ids, tbl):
    """process_aln behind -Q (which the caller applies first): True where the record is dropped"""
    c = core(r)
    if o.min_qlen > 0 and query_len(r) < o.min_qlen:
        return True
    if c["mapq"] < o.min_mapq or (c["flag"] & o.flag_on) != o.flag_on or (c["flag"] & o.flag_off):
        return True
    if o.frac > 0.:
        k = (x31(r[36:]) + o.seed) & 0xffffffff
        if (k & 0xffffff) / float(0x1000000) >= o.frac:
            return True
    if o.rg is None and ids is None and o.library is None:
        return False
    at = aux_rg(r)
    rid = None
    if at is not None:
        e = r.find(b"\0", at + 1)
        if e < 0:
            raise Undefined("an RG value runs past its record")
        rid = r[at + 1:e]
        if o.rg is not None:
            return rid != o.rg
        if ids is not None:
            return rid not in ids
    if o.library is not None:
        return rid is None or tbl.get(rid) != o.library
    return False


def number(v):
    return b"%d" % v


def fmt_g(v):
    if math.isnan(v):
        return b"-nan" if math.copysign(1.0, v) < 0 else b"nan"
    return ("%g" % v).encode()


def format_line(r, targets, style):
    """bam_format1_core with the header's names: the whole line, NULs and all, without the newline"""
    c = core(r)
    if c["l_qname"] == 0:
        raise Undefined("l_qname 0")
    cg, sq, ql, ax = layout(r)

    def target(t):
        if t >= len(targets):
            raise Undefined("a refID the header does not have")
        return targets[t][0]
    s = r[36:36 + c["l_qname"] - 1] + b"\t"
    flag = c["flag"]
    s += (number(flag) if style == 0 else b"0x%x" % flag if style == 1 else bytes(FLAG_CHARS[i] for i in range(11) if flag >> i & 1)) + b"\t"
    s += (b"*" if c["tid"] < 0 else target(c["tid"])) + b"\t" + number(to_i32(c["pos"] + 1)) + b"\t" + number(c["mapq"]) + b"\t"
    if c["n_cigar"] == 0:
        s += b"*"
    else:
        parts = []
        for w in struct.unpack_from("<%dI" % c["n_cigar"], r, cg):
            if w & 15 > 10:
                raise Undefined("a CIGAR op above 10")
            parts.append(number(w >> 4) + CIGAR_STR[w & 15:(w & 15) + 1])
        s += b"".join(parts)
    s += b"\t" + (b"*" if c["mtid"] < 0 else b"=" if c["mtid"] == c["tid"] else target(c["mtid"])) + b"\t"
    s += number(to_i32(c["mpos"] + 1)) + b"\t" + number(c["isize"]) + b"\t"
    n = c["l_qseq"]
    if n:
        s += bytes(NT16[r[sq + (i >> 1)] >> ((~i & 1) << 2) & 15] for i in range(n)) + b"\t"
        s += b"*" if r[ql] == 0xff else bytes(q + 33 & 0xff for q in r[ql:ax])
    else:
        s += b"*\t*"
    a, end = ax, len(r)
    out = [s]

    def need(k):
        if a + k > end:
            raise Undefined("an aux field runs past its record")
    while a < end:
        need(3)
        key, t = r[a:a + 2], chr(r[a + 2])
        a += 3
        out.append(b"\t" + key + b":")
        if t in WIDTH:
            w, f = WIDTH[t]
            need(w)
            out.append(b"i:" + number(struct.unpack_from(f, r, a)[0]))
            a += w
        elif t == "A":
            need(1)
            out.append(b"A:" + r[a:a + 1])
            a += 1
        elif t == "f":
            need(4)
            out.append(b"f:" + fmt_g(struct.unpack_from("<f", r, a)[0]))
            a += 4
        elif t == "d":
            need(8)
            out.append(b"d:" + fmt_g(struct.unpack_from("<d", r, a)[0]))
            a += 8
        elif t in "ZH":
            e = r.find(b"\0", a)
            if e < 0:
                raise Undefined("a string field runs past its record")
            out.append(t.encode() + b":" + r[a:e])
            a = e + 1
        elif t == "B":
            need(5)
            sub = chr(r[a])
            cnt, = struct.unpack_from("<i", r, a + 1)
            a += 5
            out.append(b"B:" + sub.encode("latin-1"))
            for _ in range(max(cnt, 0)):
                if sub in WIDTH:
                    w, f = WIDTH[sub]
                    need(w)
                    out.append(b"," + number(struct.unpack_from(f, r, a)[0]))
                    a += w
                elif sub == "f":
                    need(4)
                    out.append(b"," + fmt_g(struct.unpack_from("<f", r, a)[0]))
                    a += 4
                else:
                    out.append(b",")
        # (an unknown type: the key and a colon, and the walk goes on behind the type byte)
    return b"".join(out)


def line_length(r, targets, style, qual_scale=0):
    """the device's closed form: the bytes of the record's line with its newline, from field widths alone (integer aux types only)"""
    c = core(r)
    cg, sq, ql, ax = layout(r)
    digits = lambda v: len(str(abs(v))) + (1 if v < 0 else 0)
    name_of = lambda t: len(targets[t][0])
    flag = c["flag"]
    n = c["l_qname"] - 1 + 1
    n += (digits(flag) if style == 0 else 2 + len("%x" % flag) if style == 1 else bin(flag & 0x7ff).count("1")) + 1
    n += 2 if c["tid"] < 0 else name_of(c["tid"]) + 1
    n += digits(to_i32(c["pos"] + 1)) + 1 + digits(c["mapq"]) + 1
    n += 1 if c["n_cigar"] == 0 else sum(digits(w >> 4) + 1 for w in struct.unpack_from("<%dI" % c["n_cigar"], r, cg))
    n += 1
    n += 2 if c["mtid"] < 0 or c["mtid"] == c["tid"] else name_of(c["mtid"]) + 1
    n += digits(to_i32(c["mpos"] + 1)) + 1 + digits(c["isize"]) + 1
    L = c["l_qseq"]
    n += 3 if L == 0 else L + 1 + (1 if r[ql] == 0xff and qual_scale <= 1 else L)
    a = ax
    while a < len(r):
        t = chr(r[a + 2])
        a += 3
        n += 4
        if t in WIDTH:
            w, f = WIDTH[t]
            n += 2 + digits(struct.unpack_from(f, r, a)[0])
            a += w
        elif t == "A":
            n, a = n + 3, a + 1
        elif t in "ZH":
            e = r.index(b"\0", a)
            n, a = n + 2 + (e - a), e + 1
        elif t == "B":
            w, f = WIDTH[chr(r[a])]
            cnt, = struct.unpack_from("<i", r, a + 1)
            a += 5
            n += 3 + sum(1 + digits(v) for v in struct.unpack_from("<%d%s" % (cnt, f[1]), r, a))
            a += w * cnt
        else:
            raise ValueError(t)
    return n + 1


def text_header(text, targets):
    """samopen's -h: (bytes, stderr)"""
    n_sq = sum(1 for line in text.split(b"\0")[0].split(b"\n") if line[:4] == b"@SQ\t")
    if n_sq:
        return text, MSG_TARGETS if n_sq != len(targets) else ""
    return text + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (nm, ln) for nm, ln in targets), ""


def view(data, args, files=None, stdin=False):
    """-> (stdout, the -o file's bytes or None, stderr, status).  data: the input file's bytes (None: there is no such file);
    files: name -> bytes of the other files the arguments name"""
    o = options(args)
    err = o.err
    if o.refused or len(o.rest) > 1:
        return b"", None, None, 2
    if not o.rest:
        return b"", None, err + usage(o.long_help), 1
    if data is None:
        return b"", None, err + "open: No such file or directory\n[main_samview] fail to open \"%s\" for reading.\n" % o.rest[0], 1
    p = parse(data)
    if not p.ok:
        return b"", None, None, 2
    truncated = MSG_TRUNCATED in p.err
    err += p.err.replace(MSG_TRUNCATED, "")
    if stdin and MSG_NO_EOF not in err:      # (a finding: the check for the EOF marker cannot seek in a pipe and says the marker is absent)
        err += MSG_NO_EOF
    text, ids = p.text, None
    if o.fn_rg is not None:
        ids = set((files or {})[o.fn_rg].split())
        text = drop_rg(text, ids)
    tbl = rg_table(text) if o.library is not None else None      # (behind drop_rg: the header is parsed at the first record that asks)
    out = b""
    if not o.count and not o.bam_out and o.header:
        out, say = text_header(text, p.targets)
        err += say
    kept = []
    try:
        if not o.header_only:
            said_tbl = False
            for r in p.recs:
                r = scaled(r, o.qual_scale)
                if o.library is not None and not said_tbl and not drops_before_groups(o, r):
                    err += rg_messages(text)       # (the table is made at the first record that reaches bam_get_library)
                    said_tbl = True
                if drops(o, r, ids, tbl):
                    continue
                kept.append(r)
        lines = []
        if not o.count and not o.bam_out:
            lines = [format_line(r, p.targets, o.style).split(b"\0")[0] + b"\n" for r in kept]
    except Undefined:
        return b"", None, None, 2
    status = 1 if truncated else 0
    if truncated:
        err += MSG_TRUNC
    if o.count:
        return (b"%d\n" % len(kept) if status == 0 else b""), None, err, status
    if o.bam_out:
        blocks = cut(header_bytes(text, p.targets), kept)
        out = b"".join(member(b, o.level) for b in blocks) + EOF_BLOCK
    else:
        out += b"".join(lines)
    if o.out is None or o.out == "-":
        return out, None, err, status
    return b"", out, err, status


def drops_before_groups(o, r):
    """True where process_aln returns before it looks at the read groups"""
    import copy
    q = copy.copy(o)
    q.rg = q.library = None
    if drops(q, r, None, None):
        return True
    return (o.rg is not None or o.fn_rg is not None) and aux_rg(r) is not None


def usage(is_long):
    u = ("\nUsage:   samtools view [options] <in.bam>|<in.sam> [region1 [...]]\n\n"
         "Options: -b       output BAM\n         -h       print header for the SAM output\n         -H       print header only (no alignments)\n"
         "         -S       input is SAM\n         -u       uncompressed BAM output (force -b)\n         -1       fast compression (force -b)\n"
         "         -x       output FLAG in HEX (samtools-C specific)\n         -X       output FLAG in string (samtools-C specific)\n"
         "         -c       print only the count of matching records\n         -B       collapse the backward CIGAR operation\n"
         "         -@ INT   number of BAM compression threads [0]\n         -L FILE  output alignments overlapping the input BED FILE [null]\n"
         "         -t FILE  list of reference names and lengths (force -S) [null]\n         -T FILE  reference sequence file (force -S) [null]\n"
         "         -o FILE  output file name [stdout]\n         -R FILE  list of read groups to be outputted [null]\n"
         "         -f INT   required flag, 0 for unset [0]\n         -F INT   filtering flag, 0 for unset [0]\n"
         "         -q INT   minimum mapping quality [0]\n         -l STR   only output reads in library STR [null]\n"
         "         -r STR   only output reads in read group STR [null]\n         -s FLOAT fraction of templates to subsample; integer part as seed [-1]\n"
         "         -?       longer help\n\n")
    if not is_long:
        return u
    return u + ("Notes:\n\n  1. By default, this command assumes the file on the command line is in\n     the BAM format and it prints the alignments in SAM. If `-t' is\n"
                "     applied, the input file is assumed to be in the SAM format. The\n     file supplied with `-t' is SPACE/TAB delimited with the first two\n"
                "     fields of each line consisting of the reference name and the\n     corresponding sequence length. The `.fai' file generated by `faidx'\n"
                "     can be used here. This file may be empty if reads are unaligned.\n\n  2. SAM->BAM conversion: `samtools view -bT ref.fa in.sam.gz'.\n\n"
                "  3. BAM->SAM conversion: `samtools view in.bam'.\n\n  4. A region should be presented in one of the following formats:\n"
                "     `chr1', `chr2:1,000' and `chr3:1000-2,000'. When a region is\n     specified, the input alignment file must be an indexed BAM file.\n\n"
                "  5. Option `-u' is preferred over `-b' when the output is piped to\n     another samtools command.\n\n"
                "  6. In a string FLAG, each character represents one bit with\n     p=0x1 (paired), P=0x2 (properly paired), u=0x4 (unmapped),\n"
                "     U=0x8 (mate unmapped), r=0x10 (reverse), R=0x20 (mate reverse)\n     1=0x40 (first), 2=0x80 (second), s=0x100 (not primary), \n"
                "     f=0x200 (failure) and d=0x400 (duplicate). Note that `-x' and\n     `-X' are samtools-C specific. Picard and older samtools do not\n"
                "     support HEX or string flags.\n\n")


# ---- the device's domain and the tool's routes ----

def device_reason(recs, n_targets, o):
    """(ordinal, reason) of the first record outside the device's domain under the options o, or None"""
    text = not o.count and not o.bam_out
    groups = o.rg is not None or o.fn_rg is not None or o.library is not None
    walks = text or o.frac > 0. or o.min_qlen > 0 or o.qual_scale > 1 or groups
    plain = None
    if groups:
        import copy
        plain = copy.copy(o)
        plain.rg = plain.library = None
    for i, r in enumerate(recs):
        if not walks:
            continue
        c = core(r)
        try:
            cg, sq, ql, ax = layout(r)
        except Undefined:
            return i, R_LAYOUT
        if c["l_qname"] == 0:
            return i, R_LAYOUT
        if text or o.frac > 0.:
            nm = r[36:36 + c["l_qname"]]
            if nm.find(b"\0") != len(nm) - 1:
                return i, R_NAME
        if groups and not drops(plain, r, None, None):     # the walk to RG, for a record the filters in front let through
            try:
                at = aux_rg(r)
                if at is not None and r.find(b"\0", at + 1) < 0:
                    return i, R_LAYOUT
            except Undefined:
                return i, R_LAYOUT
        if not text:
            continue
        if c["pos"] == 0x7fffffff or c["mpos"] == 0x7fffffff:
            return i, R_POS
        if (0 <= c["tid"] and c["tid"] >= n_targets) or (0 <= c["mtid"] != c["tid"] and c["mtid"] >= n_targets):
            return i, R_TARGET
        if any(w & 15 > 9 for w in struct.unpack_from("<%dI" % c["n_cigar"], r, cg)):
            return i, R_CIGAROP
        a = ax
        while a < len(r):
            if a + 3 > len(r):
                return i, R_LAYOUT
            t = chr(r[a + 2])
            a += 3
            if t in WIDTH:
                a += WIDTH[t][0]
                if a > len(r):
                    return i, R_LAYOUT
            elif t == "A":
                if a + 1 > len(r):
                    return i, R_LAYOUT
                if r[a] == 0:
                    return i, R_ANUL
                a += 1
            elif t in "fd":
                return i, R_FLOAT
            elif t in "ZH":
                e = r.find(b"\0", a)
                if e < 0:
                    return i, R_LAYOUT
                a = e + 1
            elif t == "B":
                if a + 5 > len(r):
                    return i, R_LAYOUT
                sub = chr(r[a])
                cnt, = struct.unpack_from("<i", r, a + 1)
                a += 5
                if sub == "f":
                    return i, R_FLOAT
                if sub not in WIDTH or cnt < 0:
                    return i, R_AUXTYPE
                a += WIDTH[sub][0] * cnt
                if a > len(r):
                    return i, R_LAYOUT
            else:
                return i, R_AUXTYPE
    return None


def route(data, args, stdin=False, files=None):
    o = options(args)
    bam_to_stdout = o.bam_out and not o.count and (o.out is None or o.out == "-")
    if stdin or o.header_only or bam_to_stdout or data is None:
        return "host"
    p = parse(data)
    if not p.ok or MSG_TRUNCATED in p.err:
        return "abandoned"
    if o.library is not None:      # a header the reference has words about while it makes the ID -> LB table
        text = drop_rg(p.text, set((files or {})[o.fn_rg].split())) if o.fn_rg is not None else p.text
        if rg_messages(text):
            return "abandoned"
    for r in p.recs:         # the record index's proof refuses what lies below -1
        c = core(r)
        if c["pos"] < -1 or c["tid"] < -1 or c["mtid"] < -1 or c["mpos"] < -1:
            return "abandoned"
    return "abandoned" if device_reason(p.recs, len(p.targets), o) else "device"
