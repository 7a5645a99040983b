"""KITTI label files and annotation dicts of the offline evaluator (evaluate/kitti_common.py:293-360): text rows -> dicts of arrays
and back, the two rotated-box layouts, and the columnar form of an annotation list (SplitSide) that every whole-split launch and
both statistic paths read.

``parse_texts`` goes from the text of a whole side straight to those columns: ``device="cuda"`` through the kernels of
csrc/kitti_parse.hip, ``device="cpu"`` through a Python restatement of the same grammar (the checker).  ``_anno_from_rows`` stays the
definition: a file outside the grammar (include/prcnn_hip.h, the PRCNN_PARSE_* section) goes to it whole, a file inside gives its
bits."""
import io
import os
import pathlib
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

CLASS_CODE = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4}      # include/prcnn_hip.h: the split table


def _anno_from_rows(rows):
    """rows: list of token lists (15 or 16 tokens).  dimensions are stored l, h, w (file order h, w, l)."""
    n = len(rows)
    anno = {
        "name": np.array([r[0] for r in rows]),
        "truncated": np.array([float(r[1]) for r in rows]),
        "occluded": np.array([int(r[2]) for r in rows]),
        "alpha": np.array([float(r[3]) for r in rows]),
        "bbox": np.array([[float(v) for v in r[4:8]] for r in rows], dtype=np.float64).reshape(-1, 4),
        "dimensions": np.array([[float(v) for v in r[8:11]] for r in rows], dtype=np.float64).reshape(-1, 3)[:, [2, 0, 1]],
        "location": np.array([[float(v) for v in r[11:14]] for r in rows], dtype=np.float64).reshape(-1, 3),
        "rotation_y": np.array([float(r[14]) for r in rows]).reshape(-1),
    }
    anno["score"] = np.array([float(r[15]) for r in rows]) if n != 0 and len(rows[0]) == 16 else np.zeros([n])
    return anno


def get_label_anno(label_path):
    with open(label_path, "r") as f:
        return _anno_from_rows([line.strip().split(" ") for line in f.readlines()])


def get_label_annos(label_folder, image_ids=None):
    folder = pathlib.Path(label_folder)
    if image_ids is None:
        pat = re.compile(r"^\d{6}.txt$")
        image_ids = sorted(int(p.stem) for p in folder.glob("*.txt") if pat.match(p.name))
    if not isinstance(image_ids, list):
        image_ids = list(range(image_ids))
    return [get_label_anno(folder / ("%06d.txt" % i)) for i in image_ids]


def filter_annos_low_score(annos, thresh):
    out = []
    for a in annos:
        keep = [i for i, s in enumerate(a["score"]) if s >= thresh]
        out.append({k: v[keep] for k, v in a.items()})
    return out


def annos_from_lines(lines):
    """KITTI label lines (strings, as eval_rcnn.save_kitti_format writes them) -> annotation dict."""
    return _anno_from_rows([l.strip().split(" ") for l in lines if l.strip()])


def to_kitti_format(anno, extra=None):
    """Annotation -> the reference's 16-column %.2f text (kitti_common.py:293-304); ``extra``: a 17th column."""
    rows = []
    for i in range(len(anno["name"])):
        row = "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            anno["name"][i], anno["truncated"][i], anno["occluded"][i], anno["alpha"][i],
            anno["bbox"][i, 0], anno["bbox"][i, 1], anno["bbox"][i, 2], anno["bbox"][i, 3],
            anno["dimensions"][i, 1], anno["dimensions"][i, 2], anno["dimensions"][i, 0],
            anno["location"][i, 0], anno["location"][i, 1], anno["location"][i, 2], anno["rotation_y"][i], anno["score"][i])
        rows.append(row if extra is None else row + " %.2f" % extra[i])
    return "\n".join(rows)


def save_labels(annos, folder, ids, extras=None):
    assert len(annos) == len(ids)
    os.makedirs(folder, exist_ok=True)
    for n, (anno, i) in enumerate(zip(annos, ids)):
        with open(os.path.join(folder, "%06d.txt" % i), "w") as f:
            f.write(to_kitti_format(anno, None if extras is None else extras[n]))


def _bev_boxes(anno):
    return np.concatenate([anno["location"][:, [0, 2]], anno["dimensions"][:, [0, 2]], anno["rotation_y"][..., np.newaxis]], axis=1)


def _d3_boxes(anno):
    return np.concatenate([anno["location"], anno["dimensions"], anno["rotation_y"][..., np.newaxis]], axis=1)


def _cat(arrays, width, dtype=np.float64):
    parts = [np.asarray(a, dtype=dtype).reshape((-1, width) if width else (-1,)) for a in arrays]
    return np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, width) if width else (0,), dtype))


class SplitSide:
    """One side (labels or detections) of a split as concatenated columns: ``off`` (n_img + 1) i64 and ``off32``, the same as i32
    (what the segmented launches take), ``code`` i8 class codes of the lower-cased names (lower-casing runs over the UNIQUE names),
    ``is_dc`` (the name is exactly "DontCare"), the f64 columns named by ``keys`` (all of COLUMNS, or the fewer a caller needs and
    its annotations hold, BOX_KEYS among them), ``box3d`` = _d3_boxes and ``bev`` = _bev_boxes in f32.  ``annos``: the list given.
    A side that parse_texts made holds the columns first (``parse_stats``: files, rows, and the files the host parser read); its
    ``annos`` are built from them and the name tokens' byte spans on first access, equal to the host parser's dicts."""
    COLUMNS = {"occluded": 0, "truncated": 0, "alpha": 0, "bbox": 4, "location": 3, "dimensions": 3, "rotation_y": 0, "score": 0}      # widths
    BOX_KEYS = ("location", "dimensions", "rotation_y")
    parse_stats = None

    def __init__(self, annos, keys=tuple(COLUMNS)):
        self._annos, self.n_img = annos, len(annos)
        nums = np.array([len(a["name"]) for a in annos], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(nums)]).astype(np.int64)
        self.off32 = self.off.astype(np.int32)
        names = np.concatenate([np.asarray(a["name"], dtype=str).reshape(-1) for a in annos]) if self.n_img else np.zeros((0,), dtype=str)
        uniq, inv = np.unique(names, return_inverse=True) if names.size else (np.zeros((0,), dtype=str), np.zeros((0,), dtype=np.int64))
        self.code = np.array([CLASS_CODE.get(u.lower(), -1) for u in uniq], dtype=np.int8)[inv].reshape(-1)
        self.is_dc = np.array([u == "DontCare" for u in uniq], dtype=bool)[inv].reshape(-1)
        for key in keys:
            setattr(self, key, _cat([a[key] for a in annos], self.COLUMNS[key]))
        self._boxes()

    def _boxes(self):
        self.box3d = np.ascontiguousarray(np.concatenate([self.location, self.dimensions, self.rotation_y[:, None]], axis=1))
        self.bev = np.ascontiguousarray(self.box3d[:, [0, 2, 3, 5, 6]].astype(np.float32))

    @classmethod
    def from_columns(cls, off, code, is_dc, columns, text, name_span, host_annos, parse_stats):
        """A side from parsed columns.  text: the bytes the spans point into; name_span (n, 2) i64 offset / length of every row's name
        token (unread for the rows of ``host_annos``: file index -> the host parser's dict)."""
        self = cls.__new__(cls)
        self._annos, self.n_img = None, len(off) - 1
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.off32 = self.off.astype(np.int32)
        self.code, self.is_dc = np.ascontiguousarray(code, dtype=np.int8), np.ascontiguousarray(is_dc, dtype=bool)
        for key, width in cls.COLUMNS.items():
            setattr(self, key, np.ascontiguousarray(columns[key], dtype=np.float64).reshape((-1, width) if width else (-1,)))
        self._boxes()
        self._text, self._name_span, self._host_annos, self.parse_stats = text, name_span, host_annos, parse_stats
        return self

    @property
    def annos(self):
        if self._annos is None:
            self._annos = [self._host_annos[f] if f in self._host_annos else self._anno(f) for f in range(self.n_img)]
        return self._annos

    def _anno(self, f):
        """the dict _anno_from_rows gives for file f, from the columns"""
        a, b = int(self.off[f]), int(self.off[f + 1])
        if a == b:
            return _anno_from_rows([])
        names = [bytes(self._text[s:s + n]).decode("ascii") for s, n in self._name_span[a:b].tolist()]
        return {"name": np.array(names), "truncated": self.truncated[a:b].copy(), "occluded": self.occluded[a:b].astype(np.int64),
                "alpha": self.alpha[a:b].copy(), "bbox": self.bbox[a:b].copy(), "dimensions": self.dimensions[a:b].copy(),
                "location": self.location[a:b].copy(), "rotation_y": self.rotation_y[a:b].copy(), "score": self.score[a:b].copy()}

    def __len__(self):
        return int(self.off[-1])


class PreparedGT:
    """The ground-truth half of a split, parsed and tabulated once: pass it wherever ``gt_annos`` goes (both statistic paths take
    its columns) -- a sweep evaluates every checkpoint against the same one.  ``gt_annos``: annotation dicts, or a parsed SplitSide."""

    def __init__(self, gt_annos, ids=None):
        self.ids = None if ids is None else list(ids)
        self.side = gt_annos if isinstance(gt_annos, SplitSide) else SplitSide(list(gt_annos))

    @property
    def annos(self):
        return self.side.annos

    def __len__(self):
        return self.side.n_img


# ---- text -> columns
class ParseDeviceError(RuntimeError):
    """parse_device="cuda" was asked for and no GPU is usable.  There is no fallback to the host parser."""


PARSE_MAX_BYTES = _lib.PRCNN_PARSE_MAX_BYTES             # bytes of one device call; larger sides are cut at file boundaries
_COL = {key: getattr(_lib, "PRCNN_PARSE_" + key.upper()) for key in SplitSide.COLUMNS}
_TOKEN_COL = ([None, _COL["truncated"], _COL["occluded"], _COL["alpha"]] + [_COL["bbox"] + i for i in range(4)] +
              [_COL["dimensions"] + i for i in (1, 2, 0)] + [_COL["location"] + i for i in range(3)] + [_COL["rotation_y"], _COL["score"]])
_INT_TOKEN = re.compile(rb"[+-]?[0-9]{1,15}")
_FLOAT_TOKEN = re.compile(rb"([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]{1,9}))?")
_OUTSIDE = re.compile(rb"[^\x20-\x7e]")
_P10 = [float("1e%d" % k) for k in range(23)]                  # the exact powers of ten


def read_texts(folder, ids):
    """The files <folder>/<id as %06d>.txt as bytes, in the order of ``ids``, read on at most 16 threads"""
    def read(i):
        with open(os.path.join(folder, "%06d.txt" % i), "rb") as f:
            return f.read()
    ids = list(ids)
    if not ids:
        return []
    with ThreadPoolExecutor(max_workers=min(16, len(ids))) as pool:
        return list(pool.map(read, ids))


def _check_parse_device(parse_device):
    if parse_device not in (None, "cpu", "cuda"):
        raise ValueError("parse_device %r is neither None, 'cpu' nor 'cuda'" % (parse_device,))


def _float_token(tok):
    """A token of the regular grammar -> its f64, or None: the digits as an integer w < 10^15, then ONE multiplication or division
    by an exact power of ten, the sign last"""
    m = _FLOAT_TOKEN.fullmatch(tok)
    if m is None:
        return None
    sign, whole, frac, bare, exp = m.groups()
    digits, nfrac = (bare, len(bare)) if whole is None else (whole + (frac or b""), len(frac or b""))
    digits = digits.lstrip(b"0")
    k = int(exp or 0) - nfrac
    if len(digits) > 15 or abs(k) > 22:
        return None
    w = float(int(digits or b"0"))
    v = w * _P10[k] if k >= 0 else w / _P10[-k]
    return -v if sign == b"-" else v


def _parse_line_cpu(line, vals):
    """kitti_parse.hpp's parse_line: -> (token count | 0 blank | -1 irregular, name offset, name length)"""
    if _OUTSIDE.search(line):
        return -1, 0, 0
    body = line.strip(b" ")
    if not body:
        return 0, 0, 0
    toks = body.split(b" ")
    if len(toks) not in (15, 16):
        return -1, 0, 0
    for t, tok in enumerate(toks[1:], 1):
        v = (float(int(tok)) if _INT_TOKEN.fullmatch(tok) else None) if t == 2 else _float_token(tok)
        if v is None or not toks[0]:
            return -1, 0, 0
        vals[_TOKEN_COL[t]] = v
    return len(toks), len(line) - len(line.lstrip(b" ")), len(toks[0])


def _raw_outputs(n_rows, n_files):
    return {"vals": np.zeros((n_rows, _lib.PRCNN_PARSE_COLS)), "name_span": np.zeros((n_rows, 2), dtype=np.int64),
            "code": np.full((n_rows,), -1, dtype=np.int8), "is_dc": np.zeros((n_rows,), dtype=bool),
            "row_tok": np.zeros((n_rows,), dtype=np.uint8), "file_flag": np.zeros((n_files,), dtype=np.int32)}


def _parse_cpu(text, file_off, skip_blank):
    """The kernels' two passes in Python over text (u8 array) -> their outputs (row_off and _raw_outputs' arrays)"""
    data, n_files = text.tobytes(), len(file_off) - 1
    files = []
    for f in range(n_files):
        body = data[file_off[f]:file_off[f + 1]]
        lines, pos = [], int(file_off[f])
        for line in body.split(b"\n")[:-1] + ([body[body.rfind(b"\n") + 1:]] if body and not body.endswith(b"\n") else []):
            lines.append((pos, line))
            pos += len(line) + 1
        files.append(lines)
    row_off = np.concatenate([[0], np.cumsum([len(lines) for lines in files])]).astype(np.int64)
    out = dict(_raw_outputs(int(row_off[-1]), n_files), row_off=row_off)
    for f, lines in enumerate(files):
        for row, (pos, line) in enumerate(lines, int(row_off[f])):
            vals = [0.0] * _lib.PRCNN_PARSE_COLS
            ntok, start, length = _parse_line_cpu(line, vals)
            if ntok > 0:
                name = line[start:start + length]
                out["vals"][row], out["name_span"][row], out["row_tok"][row] = vals, (pos + start, length), ntok
                out["code"][row], out["is_dc"][row] = CLASS_CODE.get(name.lower().decode("ascii"), -1), name == b"DontCare"
            out["file_flag"][f] |= {15: _lib.PRCNN_PARSE_SAW15, 16: _lib.PRCNN_PARSE_SAW16}.get(ntok, 0 if ntok == 0 and skip_blank
                                                                                                 else _lib.PRCNN_PARSE_BAD)
    return out


def _parse_cuda(text, file_off, skip_blank, device_id):
    """csrc/kitti_parse.hip over text (u8 array): one upload, the scan, one small read of the row offsets, the parse, one read of
    every output.  All launches go to torch's current stream of the device."""
    import torch
    if not torch.cuda.is_available():
        raise ParseDeviceError("parse_device='cuda': torch sees no usable GPU (torch.cuda.is_available() is False); "
                               "there is no fallback -- pass parse_device='cpu', or None for the host parser")
    dev, n_bytes, n_files = torch.device("cuda", device_id), int(text.shape[0]), len(file_off) - 1
    if n_bytes > PARSE_MAX_BYTES or n_bytes > _lib.PRCNN_PARSE_MAX_BYTES:
        raise ValueError("one device call parses at most %d bytes, not %d" % (min(PARSE_MAX_BYTES, _lib.PRCNN_PARSE_MAX_BYTES), n_bytes))
    with torch.cuda.device(dev):
        d_text, d_off = torch.from_numpy(text).to(dev), torch.from_numpy(np.ascontiguousarray(file_off, dtype=np.int64)).to(dev)
        start_flag = torch.empty((max(1, n_bytes),), dtype=torch.uint8, device=dev)
        chunk_rows = torch.empty((-(-n_bytes // _lib.PRCNN_PARSE_CHUNK) + 1,), dtype=torch.int32, device=dev)
        d_row_off = torch.empty((n_files + 1,), dtype=torch.int64, device=dev)
        stream = _lib.current_stream(d_off)
        _lib.call("prcnn_kitti_parse_scan", n_bytes, n_files, _lib.ptr(d_text), _lib.ptr(d_off), _lib.ptr(start_flag), _lib.ptr(chunk_rows),
                  _lib.ptr(d_row_off), stream)
        row_off = d_row_off.cpu().numpy()                                        # the small read: it sizes the outputs
        n = int(row_off[-1])
        # every output in one buffer: vals | name_span | file_flag | code | is_dc | row_tok
        cols = _lib.PRCNN_PARSE_COLS
        at = np.cumsum([0, 8 * cols * n, 8 * n, 4 * n_files, n, n, n]).tolist()
        buf = torch.empty((max(1, at[-1]),), dtype=torch.uint8, device=dev)
        row_start = torch.empty((max(1, n),), dtype=torch.int32, device=dev)
        p = [buf.data_ptr() + o for o in at[:-1]]
        _lib.call("prcnn_kitti_parse_rows", n_bytes, n_files, n, int(bool(skip_blank)), _lib.ptr(d_text), _lib.ptr(d_off), _lib.ptr(start_flag),
                  _lib.ptr(chunk_rows), _lib.ptr(d_row_off), _lib.ptr(row_start), p[0], p[1], p[3], p[4], p[5], p[2], stream)
        host = buf.cpu().numpy()                                                 # the read
    part = lambda k, dtype: host[at[k]:at[k + 1]].view(dtype)
    return {"row_off": row_off, "vals": part(0, np.float64).reshape(n, cols), "name_span": part(1, np.int32).reshape(n, 2).astype(np.int64),
            "file_flag": part(2, np.int32), "code": part(3, np.int8), "is_dc": part(4, np.uint8).astype(bool), "row_tok": part(5, np.uint8)}


def _host_anno(text, skip_blank):
    """The definition on one file's text (bytes as read from the file, or str): get_label_anno's rows, or annos_from_lines' with
    skip_blank.  Raises what they raise."""
    lines = (io.TextIOWrapper(io.BytesIO(bytes(text))) if isinstance(text, (bytes, bytearray)) else io.StringIO(text, newline=None)).readlines()
    return annos_from_lines(lines) if skip_blank else _anno_from_rows([line.strip().split(" ") for line in lines])


def parse_texts(texts, device, skip_blank=False, device_id=0, host_anno=None):
    """The text of every file of one side of a split (bytes or str, in image order) -> SplitSide, without a Python float() per token.
    device "cuda": the kernels of csrc/kitti_parse.hip (no usable GPU raises ParseDeviceError: nothing falls back silently); "cpu":
    the same grammar and value rule in Python, the checker.  File semantics by default (get_label_anno: a blank line is an error of
    the host parser); skip_blank: annos_from_lines semantics, blank lines are dropped.  A file outside the regular grammar goes to the
    host parser, whole, and raises there what it raises today; ``parse_stats["host_files"]`` counts them.  ``host_anno(text,
    skip_blank)`` stands in for the host parser on those files (car_split.py: its rule accepts lines that _anno_from_rows rejects, so it
    passes one that returns no rows and decides the files named by the side's host annotations itself)."""
    if device not in ("cpu", "cuda"):
        raise ValueError("parse device %r is neither 'cpu' nor 'cuda'" % (device,))
    texts = list(texts)
    blobs = [t if isinstance(t, (bytes, bytearray)) else t.encode("utf-8", "surrogatepass") for t in texts]
    limit = min(PARSE_MAX_BYTES, _lib.PRCNN_PARSE_MAX_BYTES)
    too_long = [len(b) > limit for b in blobs]                                      # such a file is the host parser's
    blobs = [b"" if big else b for b, big in zip(blobs, too_long)]
    text = np.frombuffer(bytearray().join(blobs), dtype=np.uint8)
    file_off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    n_files, parts, f0 = len(blobs), [], 0
    while f0 < n_files or not parts:                  # one call per run of files within the limit (every file is); an empty side: one call
        f1 = min(n_files, max(f0 + 1, int(np.searchsorted(file_off, file_off[f0] + limit, side="right")) - 1))
        sub, sub_off = text[file_off[f0]:file_off[f1]], file_off[f0:f1 + 1] - file_off[f0]
        raw = _parse_cuda(sub, sub_off, skip_blank, device_id) if device == "cuda" else _parse_cpu(sub, sub_off, skip_blank)
        raw["name_span"][:, 0] += file_off[f0]
        raw["rows"] = np.diff(raw.pop("row_off"))
        parts.append(raw)
        f0 = max(f1, f0 + 1)
    raw = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    # which files are regular; which rows stay
    flag, both = raw["file_flag"], _lib.PRCNN_PARSE_SAW15 | _lib.PRCNN_PARSE_SAW16
    irregular = ((flag & _lib.PRCNN_PARSE_BAD) != 0) | ((flag & both) == both) | np.array(too_long, dtype=bool)
    file_of_row = np.repeat(np.arange(n_files), raw["rows"])
    keep = ~irregular[file_of_row] & (raw["row_tok"] != 0)
    host = {int(f): (host_anno or _host_anno)(texts[f], skip_blank) for f in np.flatnonzero(irregular)}
    host_sides = {f: SplitSide([anno]) for f, anno in host.items()}
    nums = np.bincount(file_of_row[keep], minlength=n_files).astype(np.int64)
    for f, side in host_sides.items():
        nums[f] = len(side)
    off = np.concatenate([[0], np.cumsum(nums)]).astype(np.int64)
    from_device = np.repeat(~irregular, nums)                                       # the final rows that the parser filled

    def merged(device_rows, host_rows, shape, dtype):
        if not host_sides:
            return np.ascontiguousarray(device_rows[keep], dtype=dtype)
        out = np.zeros((int(off[-1]),) + shape, dtype=dtype)
        out[from_device] = device_rows[keep]
        for f, side in host_sides.items():
            out[off[f]:off[f + 1]] = host_rows(side)
        return out

    columns = {key: merged(raw["vals"][:, _COL[key]:_COL[key] + max(1, width)].reshape((-1, width) if width else (-1,)),
                           lambda side, key=key: getattr(side, key), (width,) if width else (), np.float64)
               for key, width in SplitSide.COLUMNS.items()}
    stats = {"device": device, "files": n_files, "rows": int(off[-1]), "host_files": len(host), "calls": len(parts)}
    return SplitSide.from_columns(off, merged(raw["code"], lambda side: side.code, (), np.int8),
                                  merged(raw["is_dc"], lambda side: side.is_dc, (), bool), columns, text,
                                  merged(raw["name_span"], lambda side: 0, (2,), np.int64), host, stats)
