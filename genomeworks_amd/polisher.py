"""Polishing: a draft sequence corrected by the reads that map to it, through the three engines of this package --
cudamapper finds and aligns the overlaps, the aligned overlaps are cut into windows of the draft on the device
(cudamapper.overlap_windows), cudapoa builds the consensus of every window, and the windows are stitched.

    polished, report = polish(reads, [draft])                      # maps the reads first
    polished, report = polish(reads, [draft], overlaps=overlaps)   # overlaps of cudamapper, fused records included

The rules -- which overlap speaks for a read, which of its pieces become layers of a window, their order and number --
are in INTEGRATION.md section 3j. Windows that fewer than 2 layers span keep the draft's bases, and so do windows whose
POA does not succeed; nothing is trimmed.

    corrected, report = correct_reads(reads)                       # the reads of a set corrected with each other

polish(reads, reads) is not that: rule 1 of section 3j keeps one overlap per query read, the one with the longest
span, and for a set mapped against itself that is every read's overlap with itself, so the reads come back unchanged.
correct_reads() drops the self overlaps, keeps one record per pair of reads, aligns it once and cuts the windows of
both of its reads out of that one alignment.

    names, reads, qualities = read_fastq("reads.fastq")
    polished, report = polish(reads, [draft], read_qualities=qualities)      # layers weighted by their Phred scores
    corrected, report = correct_reads(reads, qualities=qualities)

With qualities every base of a layer enters the POA with its Phred score as its weight, and layers whose mean quality
is below min_mean_quality are dropped.

    piles = pileup(reads, [draft])                                 # uint32 (6, len(draft)): A, C, G, T, deletion, insertion
    piles = read_pileup(reads); coverage = depth(piles[0])

How every base of the draft, or of a read, is supported by the alignments polish() / correct_reads() use: per base the
number of aligned reads that put an A, C, G or T there, that delete it, and that insert after it, counted on the
device from the alignment states.

    variants = call_variants(reads, [draft])                       # SNVs, deletions, insertion alleles: a list of dicts
    text = format_vcf(variants, ["draft"], [draft])                # VCF 4.2

Where the reads disagree with the draft and what they say instead, called on the device by counting, out of the same
alignment pass as the pileup."""
import time

import numpy as np

from . import cudamapper, cudapoa


def poa_batch_shape(window_length, max_depth, band_width):
    """(max_sequence_size, max_sequences_per_poa, alignment_band_width) of the cudapoa batches polish() runs: layers
    hold up to 2 * window_length bases, a window its backbone and max_depth layers; the band as cudapoa aligns it, to a
    multiple of 128, which a batch's reads may not be shorter than."""
    band = (int(band_width) + 127) // 128 * 128
    return max(2 * int(window_length), band), int(max_depth) + 1, band


def polish(reads, targets, overlaps=None, window_length=500, max_depth=30, band_width=256, band_mode="static_band",
           devices=(0,), timings=None, poa_memory_per_device=4 << 30, read_qualities=None, target_qualities=None,
           min_mean_quality=10, **mapping_parameters):
    """`targets` polished by `reads`: (polished_targets, report). polished_targets[i] is a str, the concatenation of
    the results of target i's windows in window order: the consensus of cudapoa (scores 8 / -6 / -8, no weights,
    band_mode with band_width) over the backbone and its layers where at least 2 layers span the window and the POA's
    status is 0, the backbone otherwise. report has one dict per window, by target, then by window: target_read,
    window, layers, status (of the POA; None where it was not run) and backbone_kept.

    overlaps: OVERLAP records of reads (queries) against targets whose read ids are positions in the two lists, in
    the order cudamapper returned them; None maps first, with map_reads_batched(reads, targets, **mapping_parameters)
    over the defaults post_process=True, rescue_overlap_ends=True and filtering_parameter=1.0 -- the frequency filter
    off: map_reads_batched's own 1e-5 is meant for indices of many megabases, and in the index of a draft of a few
    hundred kilobases its threshold is 0 occurrences, so nothing would map and the draft would come back as it is;
    pass filtering_parameter for large inputs. Reads shorter than k + w - 1 then raise ValueError: the index
    would skip them and shift the read ids behind them. overlapper="chained" (and chaining=, as map_reads_batched
    takes them) is one of those mapping parameters: the overlaps then come from the chaining overlapper
    (INTEGRATION.md section 3r), and nothing else here changes. devices: the cudapoa workers' devices
    (process_windows_multi_device), each with a pool of poa_memory_per_device bytes (-1: cudapoa's share of the free
    memory, which takes seconds to set up on a large device); mapping and windows run on the current device.
    `timings`, if a dict, receives the device times (ms) chain_fuse_filter, fuse, rescue (when mapping), gather, align,
    segments, window_gather, the host times (s) map_seconds, windows_seconds, poa_seconds, stitch_seconds, and
    bytes_to_host of the windows step.

    read_qualities / target_qualities: Phred+33 strings (str / bytes), one per read and of its length, bytes in
    33..126, or None for a set without qualities, such as a FASTA draft. With either, the
    windows come from cudamapper.overlap_windows_weighted and every sequence enters the POA with its weights: c - 33
    per base, or 1 throughout for a set without qualities. With read_qualities a layer must also have a quality sum
    > 0 and a mean quality >= min_mean_quality (racon's -q). A window whose backbone weights sum to 0 keeps its
    backbone; its POA is not run and its status is None. `timings` then also receives quality_sums and weight_gather
    (device ms). With both None this is the call without qualities, and min_mean_quality is not looked at."""
    if window_length < 1:
        raise ValueError("window_length must be >= 1")
    if max_depth < 0:
        raise ValueError("max_depth must be >= 0")
    times = {} if timings is None else timings
    t0 = time.perf_counter()
    if overlaps is None:
        shortest = mapping_parameters.get("k", 15) + mapping_parameters.get("w", 10) - 1
        if any(len(r) < shortest for r in list(reads) + list(targets)):
            raise ValueError("polish: a read shorter than k + w - 1 = %d bases cannot be mapped" % shortest)
        if mapping_parameters.get("align"):
            raise ValueError("polish: the overlaps are aligned by the windows step")
        parameters = dict(dict(post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0),
                          **mapping_parameters)
        overlaps = cudamapper.map_reads_batched(reads, targets, timings=times, **parameters)
    elif mapping_parameters:
        raise TypeError("polish: mapping parameters given together with overlaps")
    t1 = time.perf_counter()
    if read_qualities is None and target_qualities is None:
        windows = cudamapper.overlap_windows(overlaps, reads, targets, window_length, max_depth, timings=times)
    else:
        windows = cudamapper.overlap_windows_weighted(overlaps, reads, targets, read_qualities, target_qualities,
                                                      window_length, max_depth, min_mean_quality, timings=times)
    t2 = time.perf_counter()
    polished, report, t3 = _consensus_of_windows(windows, len(targets), window_length, max_depth, band_width, band_mode,
                                                 devices, poa_memory_per_device)
    t4 = time.perf_counter()
    times.update(map_seconds=t1 - t0, windows_seconds=t2 - t1, poa_seconds=t3 - t2, stitch_seconds=t4 - t3)
    return polished, report


def _consensus_of_windows(windows, n_reads, window_length, max_depth, band_width, band_mode, devices,
                          poa_memory_per_device):
    """The POA of every window of overlap_windows / correction_windows that at least 2 layers span, and the results
    stitched per read: (sequences, report, the time the POA was through). Windows of the _weighted variants carry
    their weights as a fourth entry and go through the POA with them, except those whose backbone weights sum to 0."""
    weighted = bool(windows) and len(windows[0]) == 4
    deep = [i for i, w in enumerate(windows) if len(w[2]) - 1 >= 2 and (not weighted or int(w[3][0].sum()) > 0)]
    status, consensus = {}, {}
    if deep:
        size, depth, band = poa_batch_shape(window_length, max_depth, band_width)
        more = dict(weights=[windows[i][3] for i in deep]) if weighted else {}
        out = cudapoa.process_windows_multi_device([windows[i][2] for i in deep], depth, size, devices=tuple(devices),
                                                   memory_per_device=poa_memory_per_device, output_type="consensus",
                                                   band_mode=band_mode, alignment_band_width=band, gap_score=-8,
                                                   mismatch_score=-6, match_score=8, **more)
        for j, i in enumerate(deep):
            status[i], consensus[i] = int(out["status"][j]), out["consensus"][j]
    t3 = time.perf_counter()
    pieces = [[] for _ in range(n_reads)]
    report = []
    for i, (target, window, seqs) in enumerate(w[:3] for w in windows):
        kept = status.get(i) != 0
        pieces[target].append(seqs[0].decode("latin-1") if kept else consensus[i])
        report.append(dict(target_read=target, window=window, layers=len(seqs) - 1, status=status.get(i),
                           backbone_kept=kept))
    return ["".join(p) for p in pieces], report, t3


def correct_reads(reads, overlaps=None, window_length=500, max_depth=30, band_width=256, band_mode="static_band",
                  devices=(0,), timings=None, poa_memory_per_device=4 << 30, qualities=None, min_mean_quality=10,
                  **mapping_parameters):
    """`reads` corrected with each other: (corrected_reads, report), both as polish() returns them, with every read in
    the place of a target: corrected_reads[i] is the concatenation of the results of read i's windows, and report has
    one dict per window, by read, then by window, whose target_read is the read that owns the window.

    overlaps: OVERLAP records of the reads mapped against themselves, whose read ids are positions in the list, as
    cudamapper returned them -- self overlaps and both directions of a pair may be among them; None maps first, with
    map_reads_batched(reads, None, **mapping_parameters) over polish()'s defaults (overlapper="chained" among the
    parameters maps with the chaining overlapper, as there), and reads shorter than k + w - 1 raise ValueError as
    there. One record per pair of reads is aligned, once, and both of its reads get layers from it
    (cudamapper.correction_windows; the rules are in INTEGRATION.md section 3k). All windows of all reads are built
    at once, so the host holds up to (1 + max_depth) sequences of up to 2 * window_length bases per window of every
    read; reads are not corrected in batches. The remaining arguments as for polish(). `timings` receives what
    polish() gives it and pairs, overlaps_in (records aligned, records given) and query_role_segments (device ms).
    qualities: the Phred+33 strings of the reads as polish() takes them, or None; with them the windows come from
    cudamapper.correction_windows_weighted, layers are filtered by min_mean_quality and every sequence, backbones
    included, is weighted."""
    if window_length < 1:
        raise ValueError("window_length must be >= 1")
    if max_depth < 0:
        raise ValueError("max_depth must be >= 0")
    times = {} if timings is None else timings
    t0 = time.perf_counter()
    if overlaps is None:
        shortest = mapping_parameters.get("k", 15) + mapping_parameters.get("w", 10) - 1
        if any(len(r) < shortest for r in reads):
            raise ValueError("correct_reads: a read shorter than k + w - 1 = %d bases cannot be mapped" % shortest)
        if mapping_parameters.get("align"):
            raise ValueError("correct_reads: the pairs are aligned by the windows step")
        parameters = dict(dict(post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0),
                          **mapping_parameters)
        overlaps = cudamapper.map_reads_batched(reads, None, timings=times, **parameters)
    elif mapping_parameters:
        raise TypeError("correct_reads: mapping parameters given together with overlaps")
    t1 = time.perf_counter()
    if qualities is None:
        windows = cudamapper.correction_windows(overlaps, reads, window_length, max_depth, timings=times)
    else:
        windows = cudamapper.correction_windows_weighted(overlaps, reads, qualities, window_length, max_depth,
                                                         min_mean_quality, timings=times)
    t2 = time.perf_counter()
    corrected, report, t3 = _consensus_of_windows(windows, len(reads), window_length, max_depth, band_width, band_mode,
                                                  devices, poa_memory_per_device)
    t4 = time.perf_counter()
    times.update(map_seconds=t1 - t0, windows_seconds=t2 - t1, poa_seconds=t3 - t2, stitch_seconds=t4 - t3)
    return corrected, report


def _mapped(who, reads, targets, overlaps, mapping_parameters):
    """the overlaps of a pileup call: those given, or the mapping polish() / correct_reads() run, with their refusals"""
    if overlaps is not None:
        if mapping_parameters:
            raise TypeError("%s: mapping parameters given together with overlaps" % who)
        return overlaps
    shortest = mapping_parameters.get("k", 15) + mapping_parameters.get("w", 10) - 1
    if any(len(r) < shortest for r in list(reads) + list(targets or [])):
        raise ValueError("%s: a read shorter than k + w - 1 = %d bases cannot be mapped" % (who, shortest))
    if mapping_parameters.get("align"):
        raise ValueError("%s: the overlaps are aligned by the pileup step" % who)
    parameters = dict(dict(post_process=True, rescue_overlap_ends=True, filtering_parameter=1.0), **mapping_parameters)
    return cudamapper.map_reads_batched(reads, targets, **parameters)


def one_overlap_per_read(overlaps):
    """Rule 1 of INTEGRATION.md section 3j: the positions (ascending) of the overlaps polish() aligns, one per query
    read -- the one with the greatest query span, the first on ties."""
    best = {}
    for i, o in enumerate(overlaps):
        span = int(o["query_end_position_in_read"]) - int(o["query_start_position_in_read"])
        q = int(o["query_read_id"])
        if q not in best or span > best[q][0]:
            best[q] = (span, i)
    return sorted(i for _, i in best.values())


def pileup(reads, targets, overlaps=None, timings=None, **mapping_parameters):
    """How every base of `targets` is supported by the alignments polish() uses: a list with one uint32 array of shape
    (6, len(target)) per target, rows as cudamapper.PILEUP_CHANNELS -- how many aligned reads put an A, C, G or T at
    the base, how many delete it and how many insert after it. overlaps as for polish():
    None maps first, with the same defaults and the same refusals. One overlap per query read is kept (rule 1 of
    section 3j) and counted by cudamapper.overlap_pileup, which `timings` is passed to; depth(pile) is the coverage."""
    overlaps = _mapped("pileup", reads, targets, overlaps, mapping_parameters)
    kept = np.ascontiguousarray(overlaps, cudamapper.OVERLAP)
    kept = kept[one_overlap_per_read(kept)]
    return cudamapper.overlap_pileup(kept, reads, targets, timings=timings)


def read_pileup(reads, overlaps=None, timings=None, **mapping_parameters):
    """pileup() for the reads of a set mapped against itself, over the alignments correct_reads() uses: one array per
    read. overlaps as for correct_reads(): None maps first. One record per pair of reads is kept
    (cudamapper.select_pairs, rule C1 of section 3k), aligned once and counted for both of its reads
    (cudamapper.pair_pileup); self overlaps count nowhere."""
    overlaps = _mapped("read_pileup", reads, None, overlaps, mapping_parameters)
    overlaps = np.ascontiguousarray(overlaps, cudamapper.OVERLAP)
    return cudamapper.pair_pileup(overlaps[cudamapper.select_pairs(overlaps)], reads, timings=timings)


def depth(pile):
    """the coverage of every base of a pileup array: the overlaps that put a base there or delete it"""
    return pile[:5].sum(0)


def call_variants(reads, targets, overlaps=None, min_count=3, min_percent=30, timings=None, scoring=None,
                  **mapping_parameters):
    """Where the alignments polish() uses disagree with `targets`, and what they say instead: a list of dicts with
    target (position in `targets`), position (0-based), kind ("snv", "deletion", "insertion"), ref, alt, count and
    depth, by target, then by position, within a position SNV, deletion, insertion.
    overlaps as for pileup(): None maps first, with the same defaults and the same refusals; one overlap per query read
    is kept and cudamapper.overlap_variants, which `timings` is passed to, calls on the device: a count passes when it
    is >= min_count and at least min_percent per cent of the depth (both defaults are conventions, not tuned on any
    data). An SNV has the target's base as ref and the called base as alt. An insertion follows `position`; its ref is
    "" and its alt the inserted bases. Called deletions of neighbouring bases of one target are joined into one
    variant at the first of them: ref is the deleted bases, alt "", count the smallest of their counts and depth that
    of the first base. scoring, as cudamapper.overlap_variants takes it, aligns under affine gap costs instead of unit
    costs: one indel event is then one gap run in every read that carries it.
    overlapper="chained" among the mapping parameters maps with the chaining overlapper, as in polish()."""
    overlaps = _mapped("call_variants", reads, targets, overlaps, mapping_parameters)
    kept = np.ascontiguousarray(overlaps, cudamapper.OVERLAP)
    kept = kept[one_overlap_per_read(kept)]
    records = cudamapper.overlap_variants(kept, reads, targets, min_count, min_percent, timings=timings, scoring=scoring)
    return join_deletions(records, targets)


def join_deletions(records, targets):
    """the dicts call_variants() returns, from VARIANT records in their order and the targets they speak of"""
    out = []
    last, last_at = None, -1  # the deletion a next deleted base would extend: (target, the position behind it), out[]
    for v in records:
        target, p, kind = int(v["target_read"]), int(v["position"]), cudamapper.VARIANT_KINDS[int(v["kind"])]
        own = targets[target][p:p + 1]
        own = own.decode("latin-1") if isinstance(own, bytes) else own
        if kind == "deletion" and last == (target, p):
            joined = out[last_at]
            joined["ref"] += own
            joined["count"] = min(joined["count"], int(v["count"]))
            last = (target, p + 1)
            continue
        alt = ""
        if kind == "snv":
            alt = "ACGT"[int(v["alt"])]
        elif kind == "insertion":
            alt = cudamapper.insertion_allele(v["length"], v["key"])
        out.append(dict(target=target, position=p, kind=kind, ref="" if kind == "insertion" else own, alt=alt,
                        count=int(v["count"]), depth=int(v["depth"])))
        if kind == "deletion":
            last, last_at = (target, p + 1), len(out) - 1
    return out


def format_vcf(variants, target_names, targets):
    """The variants of call_variants() as VCF 4.2 text: ##fileformat, one ##contig line per target, the ##INFO lines
    of DP (depth), AD (count) and TYPE (kind), the column line, and one line per variant in target order, then by POS;
    QUAL is ".", FILTER "PASS", and there are no sample columns. An SNV stands at POS position + 1. An insertion after
    `position` stands there too, with REF the target's base and ALT that base and the inserted ones. A deletion of
    [p, p + k) with p > 0 stands at POS p with REF target[p - 1 : p + k] and ALT target[p - 1]; one of [0, k) at POS 1
    with REF target[0 : k + 1] and ALT target[k]. REF letters are as the target has them."""
    if len(target_names) != len(targets):
        raise ValueError("%d names for %d targets" % (len(target_names), len(targets)))
    texts = [t.decode("latin-1") if isinstance(t, bytes) else t for t in targets]
    lines = ["##fileformat=VCFv4.2"]
    lines += ["##contig=<ID=%s,length=%d>" % (name, len(t)) for name, t in zip(target_names, texts)]
    lines += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Aligned reads that put a base at the position or delete it">',
              '##INFO=<ID=AD,Number=1,Type=Integer,Description="Aligned reads that support the alternative allele">',
              '##INFO=<ID=TYPE,Number=1,Type=String,Description="snv, deletion or insertion">',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    rows = []
    for v in variants:
        t, p, kind = texts[v["target"]], v["position"], v["kind"]
        if kind == "snv":
            pos, ref, alt = p + 1, t[p], v["alt"]
        elif kind == "insertion":
            pos, ref, alt = p + 1, t[p], t[p] + v["alt"]
        else:
            k = len(v["ref"])
            if p + k > len(t) or (p == 0 and k >= len(t)):
                raise ValueError("a deletion of [%d, %d) of a target of %d bases has no base to stand at" % (p, p + k, len(t)))
            pos, ref, alt = (p, t[p - 1:p + k], t[p - 1]) if p > 0 else (1, t[:k + 1], t[k])
        rows.append((v["target"], pos, "%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AD=%d;TYPE=%s"
                     % (target_names[v["target"]], pos, ref, alt, v["depth"], v["count"], kind)))
    rows.sort(key=lambda r: r[:2])  # stable: the order of call_variants() within a POS
    return "\n".join(lines + [r[2] for r in rows]) + "\n"


def read_fastq(path):
    """(names, sequences, qualities) of a FASTQ file of four-line records: '@' and the name (up to the first blank),
    the bases, '+' (with or without the name repeated), and as many Phred+33 bytes, 33..126, as there are bases.
    Sequences and qualities are str. Anything else -- wrapped records, a truncated record, a missing '@' or '+', a
    length mismatch, a quality byte out of range -- raises ValueError with the line number. Empty lines at the end of
    the file are allowed. No gzip."""
    names, sequences, qualities = [], [], []
    with open(path, "rb") as f:
        lines = f.read().decode("latin-1").split("\n")
    while lines and lines[-1].strip() == "" and (len(lines) % 4 or not any(x.strip() for x in lines[-4:])):
        lines.pop()  # down to whole records: the last record may be one of no bases, whose lines are empty too
    if len(lines) % 4:
        raise ValueError("%s: %d lines are not a whole number of four-line records" % (path, len(lines)))
    for at in range(0, len(lines), 4):
        header, bases, plus, quality = (line.rstrip("\r") for line in lines[at:at + 4])
        if not header.startswith("@") or len(header.split()) < 1 or header.split()[0] == "@":
            raise ValueError("%s, line %d: a record starts with '@' and a name" % (path, at + 1))
        if not plus.startswith("+"):
            raise ValueError("%s, line %d: the third line of a record starts with '+'" % (path, at + 3))
        if len(quality) != len(bases):
            raise ValueError("%s, line %d: %d qualities for %d bases" % (path, at + 4, len(quality), len(bases)))
        if any(not 33 <= ord(c) <= 126 for c in quality):
            raise ValueError("%s, line %d: a quality byte outside 33..126" % (path, at + 4))
        if any(c.isspace() for c in bases):
            raise ValueError("%s, line %d: white space among the bases" % (path, at + 2))
        names.append(header[1:].split()[0])
        sequences.append(bases)
        qualities.append(quality)
    return names, sequences, qualities
