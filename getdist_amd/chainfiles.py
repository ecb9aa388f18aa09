"""
Chain ingestion: GetDist's plain-text chain format -- ``root_1.txt, root_2.txt, ...`` (or
``root.txt``) with columns ``weight  -log(posterior)  param_1 ... param_n``, ``root.paramnames`` (``name[*]  label``
per line, ``*`` = derived) and ``root.ranges`` (``name  lower  upper``, ``N`` = unbounded) -- read into a getdist_amd
MCSamples.  Follows chains.py:77-125 (file matching, loadNumpyTxt), chains.py:228-246 / mcsamples.py:501-528
(ignore_rows burn-in per chain, fixed-parameter deletion, makeSingle) and paramnames.py / parampriors.py for the two
side files.  A Cobaya run -- ``root.1.txt, ...`` beside ``root.updated.yaml`` -- is read the same way, its yaml standing in
for the two side files (cobaya_interface.py, read_root).  With a device context the parse itself runs on the device
(``Context.parse_text``: gd_parse_scan / gd_parse_rows, every value bit-equal to np.loadtxt); without one, or for a text the
device declines, it is host work:
pandas' C tokenizer with ``float_precision="round_trip"`` when present, else np.loadtxt.  (Measured with numpy 2.2.6 on a
161 MB file, 200 000 x 52 at ``%.8e``: np.loadtxt 1.83 s = 88 MB/s, pandas round_trip 5.18 s = 31 MB/s -- pandas is no
longer the faster of the two.)  The columns go to the device in the same SoA layout as array input.

Chain export is the way back: ``write_text_rows`` streams rows of the resident sample set into a text file whose bytes are
np.savetxt's, formatted on the device (gd_format_rows) in chunks that overlap the file writes.
"""

import os
import re

import numpy as np


def chainFiles(root, chain_indices=None, ext=".txt", separator="_", first_chain=0, last_chain=-1, chain_exclude=None):
    """chains.py:77-108: the chain files of ``root`` (``root.txt`` counts as index 0), sorted by name."""
    folder = os.path.dirname(root) or "."
    if root.endswith((os.sep, "/")):
        reg_exp = re.compile("(?P<num>[0-9]+)?" + re.escape(ext))
    else:
        reg_exp = re.compile(re.escape(os.path.basename(root)) + "(" + re.escape(separator) + "(?P<num>[0-9]+))?" + re.escape(ext))
    files = []
    for f in sorted(os.listdir(folder)):
        m = reg_exp.fullmatch(f)
        if m:
            index = int(m.group("num") or 0)
            if ((chain_indices is None or index in chain_indices) and (chain_exclude is None or index not in chain_exclude)
                    and index >= first_chain and (last_chain < 0 or index <= last_chain)):
                files.append(os.path.join(folder, f))
    return files


def patch_fixes(arr, fixes, read_token):
    """Resolves the tokens the device left undecided: ``fixes`` lists (row, field, byte offset, length), ``read_token(offset,
    length)`` returns the token's bytes, and float() -- which agrees with np.loadtxt inside the grammar the device accepts --
    gives the double that goes into ``arr[row, field]``."""
    for row, field, offset, length in fixes:
        arr[row, field] = float(bytes(read_token(offset, length)).decode("ascii"))
    return arr


def _load_text_device(fname, skiprows, parse_text, parse_args):
    """The device route of loadNumpyTxt: the (N, m) array, or None when the device declines the file."""
    res = parse_text(fname, skiprows=skiprows or 0, **parse_args)
    if res is None or res["array"].shape[1] < 3:
        return None  # np.atleast_2d(np.loadtxt) of a one-column file has a shape of its own, and read_root discards such files
    arr = res["array"]
    if len(res["fixes"]):
        with open(fname, "rb") as f:
            def read_token(offset, length):
                f.seek(offset)
                return f.read(length)

            patch_fixes(arr, res["fixes"], read_token)
    return arr


def loadNumpyTxt(fname, skiprows=None, ctx=None, _parse_args=None):
    """chains.py:115-125: a 2D float array from a whitespace-separated text file (``#`` comments allowed).

    With a context that can parse (``ctx.parse_text``: the device context, not the numpy test double) the text is copied to
    the device in chunks and parsed there, bit-equal to np.loadtxt; the few tokens the device cannot decide come back as
    a list and are converted here.  Whatever the device declines -- a ragged or otherwise not plain text, skipped lines
    that hold a lone CR or bytes outside ASCII (only a text-mode reader counts and decodes them as the reference does),
    fewer than 3 columns, a short fix list, a file too large for the free device memory -- takes the host route below for the whole
    file, so the values and the ValueError of a half-written file are the reference parser's own.  ``_parse_args`` are
    keyword arguments for parse_text (tests cut the file into small chunks with it)."""
    if os.path.getsize(fname) == 0:
        return np.zeros((0, 0))
    parse_text = getattr(ctx, "parse_text", None)
    if parse_text is not None:
        arr = _load_text_device(fname, skiprows, parse_text, _parse_args or {})
        if arr is not None:
            return arr
    try:
        import pandas as pd

        # round_trip: correctly rounded decimal -> double, bit-equal to np.loadtxt (the default fast parser is not)
        df = pd.read_csv(fname, sep=r"\s+", header=None, comment="#", skiprows=skiprows or 0, dtype=np.float64,
                         engine="c", float_precision="round_trip")
        arr = np.atleast_2d(df.to_numpy())
        if np.isnan(arr).any():
            # pandas pads a short row with NaN where np.loadtxt -- the reference -- raises: a chain file that is still
            # being written must fail loudly, not yield a NaN sample (and poison the binary cache).  NaN written in the
            # file itself parses identically in np.loadtxt, which then decides.
            # (a ValueError of the reference's parser is reported once, by the handler below: chains.py:121-125)
            return np.atleast_2d(np.loadtxt(fname, skiprows=skiprows or 0))
        return arr
    except ImportError:
        return np.atleast_2d(np.loadtxt(fname, skiprows=skiprows or 0))
    except ValueError:
        print("Error reading %s" % fname)
        raise


def readParamNames(fname, with_comments=False):
    """paramnames.py:97-111, 250-270: (names, labels, derived flags[, comments]) of a .paramnames file; what follows a
    ``#`` on a line is the parameter's comment (ParamInfo.string writes it there), not part of the label."""
    names, labels, derived, comments = [], [], [], []
    with open(fname, encoding="utf-8-sig") as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            parts = line.split(None, 1)
            name = parts[0]
            is_derived = name.endswith("*")
            names.append(name[:-1] if is_derived else name)
            derived.append(is_derived)
            label, _, comment = parts[1].partition("#") if len(parts) > 1 else ("", "", "")
            labels.append(label.strip() or None)
            comments.append(comment.strip())
    return (names, labels, derived, comments) if with_comments else (names, labels, derived)


def readRanges(fname):
    """parampriors.py:30-60, 89-94: name -> (lower, upper) with None for 'N'; (lower, upper, True) for a line with a fourth
    field that says periodic (what ParamBounds.__str__ writes behind a periodic parameter)."""
    ranges = {}
    with open(fname, encoding="utf-8-sig") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 3 and not parts[0].startswith("#"):
                lo, hi = (None if v in ("N", "None") else float(v) for v in parts[1:3])
                periodic = len(parts) == 4 and parts[3].upper() in ("T", "TRUE", "PERIODIC")
                ranges[parts[0]] = (lo, hi, True) if periodic else (lo, hi)
    return ranges


TEXT_CHUNK_BYTES = 192 << 20  # text per chunk of write_text_rows: two device and two page-locked blocks of this size
_DEVICE_SPEC = re.compile(r"%([1-9][0-9]*)?(?:\.([0-9]+))?([eE])")
_host_route_logged = set()


def parse_device_format(fmt):
    """(width, prec, upper) when ``fmt`` is one ``%[width][.prec](e|E)`` conversion without flags, inside the range the
    device formats (width <= 32, prec <= 17; no precision means 6, as in C) -- ``"%.8e"`` (chains.py:227) and ``"%16.7E"``
    (mcsamples.py:598) among them; None for anything else (%f, %g, flags, a list of formats), which np.savetxt formats
    on the host."""
    from ._lib import GD_FMT_MAX_PREC, GD_FMT_MAX_WIDTH

    m = _DEVICE_SPEC.fullmatch(fmt) if isinstance(fmt, str) else None
    if m is None:
        return None
    width, prec = int(m.group(1) or 0), 6 if m.group(2) is None else int(m.group(2))
    if width > GD_FMT_MAX_WIDTH or prec > GD_FMT_MAX_PREC:
        return None
    return width, prec, m.group(3) == "E"


def _write_rows_host(f, rows, fmt, delimiter, host_rows, why):
    """The documented host route: np.savetxt of the rows gathered on the host -- the reference's own code path."""
    import logging

    if why not in _host_route_logged:
        _host_route_logged.add(why)
        logging.getLogger(__name__).info("chain text is formatted on the host by np.savetxt: %s", why)
    if isinstance(rows[0], (int, np.integer)):
        index = slice(int(rows[0]), int(rows[1]))
    else:
        buf, K = rows
        index = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
    np.savetxt(f, host_rows(index), fmt=fmt, delimiter=delimiter)


def _write_rows_device(f, ctx, srcs, rows, spec, sep, chunk_rows):
    import queue
    import threading

    from ._lib import format_field_bytes

    width, prec, upper = spec
    contiguous = isinstance(rows[0], (int, np.integer))
    total = int(rows[1]) - int(rows[0]) if contiguous else int(rows[1])
    if total <= 0:
        return
    per_row = len(srcs) * format_field_bytes(width, prec)
    chunk_rows = int(chunk_rows) if chunk_rows else max(1, TEXT_CHUNK_BYTES // per_row)
    chunk_rows = min(chunk_rows, total)
    nbuf = 2 if total > chunk_rows else 1
    dev = [ctx.alloc(chunk_rows * per_row) for _ in range(nbuf)]
    host = [ctx.pinned_array((chunk_rows * per_row,), np.uint8) for _ in range(nbuf)]
    free, todo, failed = queue.Queue(), queue.Queue(), []
    for b in range(nbuf):
        free.put(b)

    def drain():  # waits for a chunk's copy and writes it while the next chunk is formatted and copied
        ctx.bind_thread()
        while True:
            item = todo.get()
            if item is None:
                return
            b, nbytes, mark = item
            try:
                if not failed:
                    ctx.copy_wait(mark)
                    f.write(memoryview(host[b])[:nbytes])
            except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread below
                failed.append(e)
            finally:
                free.put(b)

    writer = threading.Thread(target=drain, name="getdist_amd-text-writer")
    writer.start()
    try:
        for start in range(0, total, chunk_rows):
            b = free.get()
            if failed:
                break
            k = min(chunk_rows, total - start)
            if contiguous:
                _, nbytes = ctx.format_rows(srcs, lo=int(rows[0]) + start, hi=int(rows[0]) + start + k, width=width, prec=prec,
                                            upper=upper, sep=sep, out=dev[b])
            else:
                _, nbytes = ctx.format_rows(srcs, rows=rows[0], K=k, row_offset=start, width=width, prec=prec, upper=upper,
                                            sep=sep, out=dev[b])
            ctx.fetch_bytes_async(dev[b], host[b], nbytes)
            todo.put((b, nbytes, ctx.copy_mark()))
    finally:
        todo.put(None)
        writer.join()
        for d in dev:
            d.free()
    if failed:
        raise failed[0]


def write_text_rows(path_or_file, ctx, srcs, rows, fmt="%.8e", delimiter=" ", chunk_rows=None, host_rows=None):
    """
    np.savetxt(path_or_file, <rows of the resident sample set>, fmt=fmt, delimiter=delimiter) without the host loop
    (chains.py:1081-1085: one Python ``%`` per number there).  Field j of a row is ``srcs[j]``: a resident column (spare
    columns included) or one of the GD_FMT_SRC_* codes of gd_format_rows; ``rows`` is ``(lo, hi)`` or ``(device int32 row
    list, K)``.  The text is formatted on the device in chunks of ``chunk_rows`` rows (default: TEXT_CHUNK_BYTES of text)
    into two device blocks, copied into two page-locked blocks on the copy stream and written by a helper thread, so the
    ``file.write`` of one chunk overlaps the kernels and the copy of the next.  Zero rows give an empty file.

    A path is written as ``path + ".tmp<pid>"`` and renamed when complete (as write_soa_cache): an interrupted save leaves
    no truncated chain that a later load would take for a whole one.  An open binary file is written in place.

    Host route: a format the device does not take (parse_device_format), a delimiter other than "" / " ", or a context
    that cannot format (the numpy test double of the CPU tier) is written by np.savetxt itself from ``host_rows(index)``,
    the (rows, m) host array of a slice or an index array; one logging line says so.
    """
    spec = parse_device_format(fmt)
    why = None
    if spec is None:
        why = "format %r is not a single %%[width][.prec]e conversion" % (fmt,)
    elif delimiter not in ("", " "):
        why = "delimiter %r" % (delimiter,)
    elif not hasattr(ctx, "format_rows"):
        why = "the context has no device formatter"
    if why is not None and host_rows is None:
        raise ValueError("cannot write rows on the host route (%s) without host_rows" % why)

    def body(f):
        if why is not None:
            _write_rows_host(f, rows, fmt, delimiter, host_rows, why)
        else:
            _write_rows_device(f, ctx, srcs, rows, spec, delimiter == " ", chunk_rows)

    if hasattr(path_or_file, "write"):
        body(path_or_file)
        return
    path = os.fspath(path_or_file)
    tmp = path + ".tmp%d" % os.getpid()
    try:
        with open(tmp, "wb") as f:
            body(f)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def read_properties(fname):
    """The flat ``key=value`` lines of a .properties.ini (inifile.py:70-105 without includes): {key: value string}."""
    params = {}
    with open(fname, encoding="utf-8-sig") as f:
        for line in f:
            s = line.strip()
            if s == "END":
                break
            if not s or s.startswith("#"):
                continue
            eq = s.find("=")
            if eq >= 0:
                params[s[:eq].strip()] = s[eq + 1:].strip()
    return params


def write_properties(fname, params, read_order=()):
    """inifile.py:130-166 for a file without includes: ``key=value`` lines -- first the keys of ``read_order`` (the order
    of the file the values were read from), then the others sorted -- joined by newlines without a trailing one,
    booleans as T / F."""
    def text(v):
        return v if isinstance(v, str) else str(v)[0] if isinstance(v, bool) else str(v)

    keys = [k for k in read_order if k in params]
    keys += sorted(k for k in params if k not in keys)
    with open(fname, "w", encoding="utf-8") as f:
        f.write("\n".join(k + "=" + text(params[k]) for k in keys))


CACHE_MAGIC = b"GDAMDSOA1\n"
CACHE_ALIGN = 4096


def cache_path(file_root):
    return file_root + ".gdamd_soa"


def write_soa_cache(path, chains):
    """
    Binary chain cache (the role of the reference's ``.py_mcsamples`` pickle, mcsamples.py:83-126, in a layout made for
    the device): magic, one JSON header line (rows per chain, columns), zero padding to a 4096-byte boundary, then the
    stacked chain rows as ONE column-major fp64 block -- column 0 = weight, 1 = -log(posterior), 2.. = parameters --
    i.e. exactly the SoA layout of the device (ctx.hpp), so a load is one sequential read into page-locked memory
    followed by per-column DMA with no transpose and no text parse.
    """
    import json

    rows = [int(c.shape[0]) for c in chains]
    ncol = int(chains[0].shape[1])
    head = json.dumps(dict(rows=rows, ncol=ncol, dtype="<f8")).encode() + b"\n"
    pad = (-(len(CACHE_MAGIC) + len(head))) % CACHE_ALIGN
    tmp = path + ".tmp%d" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(CACHE_MAGIC + head + b"\0" * pad)
        for j in range(ncol):
            for c in chains:
                np.ascontiguousarray(c[:, j], dtype="<f8").tofile(f)
    os.replace(tmp, path)


def read_soa_cache(path, alloc=None):
    """(column-major (N, ncol) array, rows per chain) from a cache file.  ``alloc(shape, dtype)`` supplies the host
    buffer (page-locked memory from the device context); the file is read straight into it."""
    import json

    with open(path, "rb") as f:
        if f.read(len(CACHE_MAGIC)) != CACHE_MAGIC:
            raise ValueError("not a getdist_amd chain cache: " + path)
        head = json.loads(f.readline().decode())
        pos = f.tell()
        f.seek(pos + (-pos) % CACHE_ALIGN)
        N, ncol = int(sum(head["rows"])), int(head["ncol"])
        flat = alloc((N * ncol,), np.float64) if alloc is not None else np.empty(N * ncol)
        got = f.readinto(memoryview(flat).cast("B"))
        if got != N * ncol * 8:
            raise ValueError("truncated chain cache: " + path)
    return flat.reshape((ncol, N)).T, head["rows"]


def read_root(file_root, chain_exclude=None, no_cache=False, alloc=None, ctx=None):
    """
    Everything ``MCSamples(root=...)`` / ``loadMCSamples`` read from disk (mcsamples.py:47-146, chains.py:1368-1405):
    the chain files (or the binary cache when it is newer than all of them), ``.paramnames`` and ``.ranges``.
    Returns dict(samples=[per-chain (rows, n)], weights=[...], loglikes=[...], names, labels, derived, ranges,
    from_cache).  No burn-in is removed here.  ``ctx`` parses the chain files on the device (loadNumpyTxt).

    A root without ``.paramnames`` beside which cobaya_interface.cobaya_params_file finds a yaml is a Cobaya run
    (``root.1.txt, ...``): names, labels, derived flags and ``renames`` come from the yaml, matched to the chain columns by
    position, and -- unless ``root.ranges`` exists -- so do the ranges, of every parameter the yaml lists (a fixed parameter
    has no column; the ranges of a GetDist-format root are restricted to its columns).  ``info_dict`` is the parsed yaml
    (None for any other root).  The cache of such a root is also older than any ``*updated.yaml`` / ``*full.yaml`` with
    the root's prefix.
    """
    from .chains import WeightedSampleError

    files = chainFiles(file_root, chain_exclude=chain_exclude) or chainFiles(file_root, separator=".", chain_exclude=chain_exclude)
    if not files:
        raise OSError("No chains found: " + file_root)
    if chain_exclude:
        no_cache = True  # mcsamples.py:73-74
    cpath = cache_path(file_root)
    chains = None
    from_cache = False
    getdist_format = os.path.isfile(file_root + ".paramnames")
    sources = list(files)
    if not getdist_format:
        # mcsamples.py:95-101: a Cobaya run's cache is also older than any yaml of the run written since (a resumed or
        # post-processed run rewrites updated.yaml; the chain rows it describes may have changed with it)
        folder, prefix = os.path.dirname(file_root) or ".", os.path.basename(file_root)
        sources += [os.path.join(folder, f) for f in os.listdir(folder)
                    if f.startswith(prefix) and f.lower().endswith(("updated.yaml", "full.yaml"))]
    if not no_cache and os.path.isfile(cpath) and max(os.path.getmtime(f) for f in sources) < os.path.getmtime(cpath):
        try:
            block, rows = read_soa_cache(cpath, alloc)
            offs = np.cumsum([0] + list(rows))
            chains = [block[a:b] for a, b in zip(offs[:-1], offs[1:])]
            from_cache = True
        except (ValueError, OSError, KeyError):
            chains = None
    if chains is None:
        chains = []
        for fname in files:
            cols = loadNumpyTxt(fname, ctx=ctx)
            if cols.shape[0] == 0 or cols.shape[1] < 3:
                continue  # "Ignored file (likely empty)" (chains.py:1400-1403)
            chains.append(cols)
        if not chains:
            raise WeightedSampleError("loadChains - no chains found for " + file_root)
        if not no_cache:
            try:
                write_soa_cache(cpath, chains)
            except OSError:
                pass  # read-only chain directory: the cache is an optimisation only
    n = chains[0].shape[1] - 2
    labels = derived = comments = renames = info_dict = None
    yaml_file = None
    if getdist_format:
        names, labels, derived, comments = readParamNames(file_root + ".paramnames", with_comments=True)
        if len(names) != n:
            raise WeightedSampleError("paramnames file does not match the number of chain columns")
    else:
        from .cobaya_interface import cobaya_params_file

        yaml_file = cobaya_params_file(file_root)
        if yaml_file:
            # chains.py:1131-1136: a Cobaya run.  Its parameters are matched to the chain columns by position (the header
            # line of the chain files is a comment to the parser): sampled first, then derived (ParamNames.loadFromFile)
            from .paramnames import ParamNames

            pars = ParamNames.fromFile(yaml_file)
            names, labels = pars.list(), pars.labels()
            if len(names) != n:
                raise WeightedSampleError("the parameters of %s do not match the number of chain columns" % os.path.basename(yaml_file))
            derived = [p.isDerived for p in pars.names]
            renames, info_dict = pars.getRenames(), pars.info_dict
        else:
            names = ["param%d" % (i + 1) for i in range(n)]
    if os.path.isfile(file_root + ".ranges"):  # mcsamples.py:2280-2291: the .ranges file, else the run's yaml
        ranges = readRanges(file_root + ".ranges")
        if yaml_file is None:
            ranges = {k: v for k, v in ranges.items() if k in names}
    elif yaml_file:
        from .cobaya_interface import get_info_params, get_range

        # every entry, not only the chain's columns: a fixed parameter has no column and is a zero-width range
        ranges = {p: get_range(entry) for p, entry in get_info_params(info_dict).items()}
    else:
        ranges = {}
    return dict(samples=[c[:, 2:] for c in chains], weights=[c[:, 0] for c in chains], loglikes=[c[:, 1] for c in chains],
                names=names, labels=labels, derived=derived, comments=comments, ranges=ranges, renames=renames,
                info_dict=info_dict, from_cache=from_cache)


def loadMCSamples(file_root, ini=None, jobItem=None, no_cache=False, settings=None, chain_exclude=None, **kwargs):
    """
    mcsamples.py:47-126: an MCSamples from the chain files of ``file_root`` (``ignore_rows`` burn-in per chain --
    a row count if >= 1, else a fraction --, per-chain minimum-weight filter, deletion of the parameters that do not
    move, names / labels / derived flags and hard bounds from the side files).  The first load writes the binary
    column cache next to the chains; later loads stream it (``no_cache`` or ``chain_exclude`` bypass it, as in the
    reference).
    """
    from .mcsamples import MCSamples

    if jobItem is not None:
        raise NotImplementedError("grid job items are outside the accelerated path")
    return MCSamples(root=file_root, ini=ini, settings=settings, _chain_exclude=chain_exclude, _no_cache=no_cache, **kwargs)
