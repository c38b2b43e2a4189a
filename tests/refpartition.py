"""selectReads' partitioned branch restated on the CPU from the reference's source (apps/FilterReads.h:209-278,
src/ReadSelector.h:513-596, 1212-1262): the sequence of rounds, availability, the remainder condition, the pair decision, the
order of the output and the names of the files.  Helper of the partition tests; nothing here is derived from the device code."""
import bisect

import numpy as np


U32 = 0xffffffff
SUFFIX = {False: ".fastq", True: ".fasta"}          # FormatOutput::getSuffix, src/Utils.h:132-142


def round_table(min_depth, partition_by_depth, remainder_trim=-1.0, min_read_length=0.40, min_passing_in_pair=1):
    """The loop of apps/FilterReads.h:211-272 with its unsigned arithmetic: a list of rounds in the order they run, each
    dict(depth=tmpMinDepth, min_read_length, both_pass, is_remainder).  partition_by_depth <= 0 = not partitioned."""
    min_depth &= U32
    max_depth = partition_by_depth                     # int maxDepth = getPartitionByDepth()            :211
    is_partitioned = max_depth > 0                     #                                                 :212
    if not is_partitioned:
        max_depth = min_depth                          #                                                 :213-215
    mrl = float(np.float32(min_read_length))           # float oldMinReadLength                          :217
    has_remainder = False
    rounds = []
    depth = max_depth & U32                            # unsigned int depth = maxDepth                   :221
    while depth >= min_depth:
        tmp_min_depth = float(np.float32(max(min_depth, depth)))                                       # :223
        rounds.append(dict(depth=tmp_min_depth, min_read_length=mrl, both_pass=min_passing_in_pair == 2, is_remainder=has_remainder))
        if depth == min_depth:                                                                         # :256
            if (not has_remainder and is_partitioned and remainder_trim > 0.0
                    and (min_passing_in_pair != 1 or float(int(mrl)) != float(np.float32(remainder_trim)))):     # :257-262
                min_passing_in_pair = 1                                                                # :264
                mrl = float(np.float32(remainder_trim))                                                # :265
                has_remainder = True
                depth = (depth * 2) & U32                                                              # :267
            else:
                break                                                                                  # :269
        depth //= 2                                                                                    # :221
    return rounds


def passes_length(length, read_length, minimum_length):
    """ReadSelectorUtil::passesLength (src/ReadSelector.h:209-228) in the float arithmetic of the reference: readLength *
    minimumLength is an integer times a float, rounded to float before it is compared (5 x 0.40f is exactly 2, so a trim of 2 of
    5 bases passes; in double the product lies just above 2)"""
    f = np.float32
    if f(length) <= f(1.0):
        return False
    if f(minimum_length) <= f(1.0):
        return bool(f(read_length) * f(minimum_length) <= f(length))
    return bool(f(minimum_length) <= f(length))


def output_name(output, min_depth, rnd, is_partitioned, separate_outputs=True):
    """the name selectReads hands getOFM for one round (:170-176, 228-234), before writePick's per-input key"""
    name = output
    if separate_outputs:
        name += "-MinDepth%d" % min_depth                                                              # :173
        if rnd["is_remainder"]:
            name += "-Remainder"                                                                       # :230
        elif is_partitioned and rnd["depth"] > 0:
            name += "-PartitionDepth%.9g" % rnd["depth"]      # lexical_cast<string>(float): 16, not 16.0   :232
    return name


def file_name(output, min_depth, rnd, is_partitioned, prefix, separate_outputs=True, fasta=False):
    """OfstreamMap: prefix + key + suffix (src/Utils.h:421-426); key = "-" + getReadFileNamePrefix(read) and the suffix is the
    format's only with --separate-outputs (src/ReadSelector.h:1256-1259, apps/FilterReads.h:171-176)"""
    if not separate_outputs:
        return output
    return output_name(output, min_depth, rnd, is_partitioned) + "-" + prefix + SUFFIX[bool(fasta)]


def record_text(name, seq, qual, label, discarded, to, tl, shift, out_base, fasta):
    """Read::toFastq / toFasta (src/Sequence.cpp:761-779): a discarded read or a trim of at most one base prints as N with the
    quality out_base + 1 (src/Sequence.cpp:305-311, 729-733)"""
    tl = 0 if discarded else min(int(tl), max(0, len(seq) - int(to)))
    if discarded or tl <= 1:
        s, q = b"N", bytes([out_base + 1])
    else:
        s = seq[int(to):int(to) + tl]
        q = bytes((c + shift) & 0xff for c in qual[int(to):int(to) + tl])
    head = name + ((b" " + label) if label else b"")
    return (b">" + head + b"\n" + s + b"\n") if fasta else (b"@" + head + b"\n" + s + b"\n+\n" + q + b"\n")


def partition(names, seqs, quals, labels, disc, to, tl, sc, mate, rounds, input_starts=None, shift=0, out_base=33, fasta=False):
    """The rounds over one read set.  isPassingRead asks for trim.isAvailable (:554); a pair passes with both reads or either
    (:558-568); every read of a passing pair is picked and made unavailable (pickIfNew :513-542, pickAllPassingPairs :585-596;
    mate None or -1 = pickAllPassingReads :576-583); the picks of the round are sorted (optimizePickOrder :1212-1221) and written,
    each to the file of its input (writePick :1252-1262).  Returns (text, table, read_segment): the concatenation of the
    segments round-major then by input, table[round][input] = (first pick, picks, first byte, bytes), and per read
    round * n_inputs + input or -1."""
    n = len(names)
    starts = [0, n] if input_starts is None else [int(x) for x in input_starts]
    n_inputs = len(starts) - 1
    available = [True] * n
    lens = [len(s) for s in seqs]
    sc32 = np.asarray(sc, dtype=np.float32)
    read_segment = np.full(n, -1, dtype=np.int32)
    out, table = [], []
    n_picks = n_bytes = 0
    for r, rnd in enumerate(rounds):
        depth, mrl = np.float32(rnd["depth"]), rnd["min_read_length"]

        def passing(i):
            return (not disc[i]) and available[i] and bool(sc32[i] >= depth) and passes_length(float(tl[i]), lens[i], mrl)
        picks = []
        for i in range(n):
            j = -1 if mate is None else int(mate[i])
            if j < 0:
                ok = passing(i)
            else:
                ok = (passing(i) and passing(j)) if rnd["both_pass"] else (passing(i) or passing(j))
            if ok:
                picks.append(i)
        for i in picks:
            available[i] = False
        row = []
        for f in range(n_inputs):
            mine = [i for i in picks if bisect.bisect_right(starts, i) - 1 == f] if n_inputs > 1 else picks
            text = b"".join(record_text(names[i], seqs[i], quals[i], labels[i], disc[i], to[i], tl[i], shift, out_base, fasta) for i in mine)
            for i in mine:
                read_segment[i] = r * n_inputs + f
            row.append((n_picks, len(mine), n_bytes, len(text)))
            n_picks += len(mine)
            n_bytes += len(text)
            out.append(text)
        table.append(row)
    return b"".join(out), table, read_segment
