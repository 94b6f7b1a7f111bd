"""An independent byte-level restatement of Flink's wire format, in plain Python (struct, int; numpy only for the
float32 rounding and for the returned columns).  It loads neither liboracle nor the library: tests compare BOTH with
it (test_oracle_wire_edges.py vets oracle/wire_oracle.cpp, test_gpu_wire_edges.py the kernels of fw_wire.hip).

Written from the reference's sources:
  * SpanningRecordSerializer.java:76-98 (flink-runtime/.../io/network/api/serialization): every element is written
    as `lengthBuffer.putInt(0, len)` -- a 4-byte big-endian length -- followed by its `len` bytes.
  * StreamElementSerializer.java:167-197 (flink-streaming-java/.../runtime/streamrecord), serialize(): one tag byte,
    0 record with timestamp (writeLong timestamp, then the value), 1 record without timestamp (the value),
    2 watermark (writeLong), 3 latency marker (writeLong marked time, writeLong lower part, writeLong upper part,
    writeInt subtask), 4 stream status (writeInt).  :199-221 deserialize(): `int tag = source.readByte()` (a SIGNED
    byte), any other tag throws IOException("Corrupt stream, found tag: " + tag).
  * DataOutputSerializer.java:173-175 writeDouble = writeLong(Double.doubleToLongBits(v)), :178-180 writeFloat =
    writeInt(Float.floatToIntBits(v)) -- both collapse every NaN to the canonical 0x7ff8000000000000 / 0x7fc00000 --
    and :184-215 writeInt / writeLong / writeShort: big-endian two's complement.
  * StringValue.java:745-787 readString and :789-817 writeString: length + 1 as a base-128 varint, low group first
    (0 = null), then every UTF-16 char as such a varint; readString casts each decoded int to (char).
  * TimeWindow.java:83-85 maxTimestamp() = end - 1 (Java long arithmetic: it wraps), GlobalWindow.java:45-46
    maxTimestamp() = Long.MAX_VALUE.
TupleSerializer writes a Tuple's fields in order with no null mask, so a value is its fields back to back.

What is this build's own choice rather than the reference's (include/flink_window.h documents each):
  * the operator's columns: integers sign-extended to 64 bits, Boolean 0 / 1, Double as its bits, Float widened to
    double bits (the payload of a widened NaN is not pinned: compare those by class);
  * a String key's 64-bit id (FNV-1a 64 over the UTF-16 chars, then fmix64 of it ^ the length) beside String.hashCode;
  * a null String key is refused (code -4), an element whose length differs from what its tag and the layout give is
    refused (-2), an empty element is refused (-3: readByte at the end of the input);
  * a record with String fields longer than 64 bytes with its prefix is refused (-2; decode's `string_limit`), and
    so is a varint whose fifth byte still has its continuation bit (writeString never writes one: an int has five
    base-128 groups);
  * encode: an f64 row field written into an integer field is Java's `(long) d`, then the field's low bytes; an
    integer row field written into a Double / Float field is `(double) v`, then `(float)` of that.
"""
import struct

import numpy as np

LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
SIZE = {"long": 8, "double": 8, "int": 4, "float": 4, "short": 2, "byte": 1, "boolean": 1}
ROW_FIELDS = ("key", "start", "end", "count", "sum", "min", "max")
CANON_NAN64, CANON_NAN32 = 0x7ff8000000000000, 0x7fc00000


def _be(v, nb):
    """DataOutputSerializer.writeLong / writeInt / writeShort / write: the low nb bytes, most significant first."""
    return (int(v) & ((1 << (8 * nb)) - 1)).to_bytes(nb, "big")


def _signed(u, bits):
    u &= (1 << bits) - 1
    return u - (1 << bits) if u >> (bits - 1) else u


def double_from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & ((1 << 64) - 1)))[0]


def bits_from_double(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def is_nan64(b):
    return (b & 0x7ff0000000000000) == 0x7ff0000000000000 and (b & 0x000fffffffffffff) != 0


def is_nan32(b):
    return (b & 0x7f800000) == 0x7f800000 and (b & 0x007fffff) != 0


def double_to_long_bits(b):
    """Double.doubleToLongBits on a bit pattern: every NaN becomes 0x7ff8000000000000."""
    b &= (1 << 64) - 1
    return CANON_NAN64 if is_nan64(b) else b


def float_to_int_bits_of_double(b):
    """Float.floatToIntBits((float) d) for the double of bits b: round to nearest even, every NaN 0x7fc00000."""
    if is_nan64(b):
        return CANON_NAN32
    with np.errstate(over="ignore", under="ignore"):
        f = np.array([double_from_bits(b)], dtype=np.float64).astype(np.float32)
    return int(f.view(np.uint32)[0])


def java_long_cast(b):
    """Java's (long) d (JLS 5.1.3): NaN -> 0, beyond the range -> Long.MAX_VALUE / MIN_VALUE, else toward zero."""
    if is_nan64(b):
        return 0
    d = double_from_bits(b)
    if d >= 9223372036854775808.0:
        return LONG_MAX
    if d <= -9223372036854775808.0:
        return LONG_MIN
    return int(d)


# ---- writing --------------------------------------------------------------------------------------------------
def _varint(v):
    out = bytearray()
    while v >= 0x80:  # out.write(v | HIGH_BIT); v >>>= 7
        out.append((v | 0x80) & 0xff)
        v >>= 7
    out.append(v)
    return bytes(out)


def utf16_units(s):
    if isinstance(s, str):
        e = s.encode("utf-16-le", "surrogatepass")
        return [e[i] | (e[i + 1] << 8) for i in range(0, len(e), 2)]
    return [int(c) for c in s]


def write_string(s):
    """StringValue.writeString (StringValue.java:789-817).  s: a str, a sequence of UTF-16 units, or None."""
    if s is None:
        return b"\x00"
    u = utf16_units(s)
    return _varint(len(u) + 1) + b"".join(_varint(c) for c in u)


def put_field(kind, x):
    """One field.  Integer kinds: an int (its low bytes are written).  double / float: a Python float is written as
    the reference does (doubleToLongBits / floatToIntBits of its float rounding); an int is the field's raw bits,
    written verbatim (bytes no Java writer produces, which a decoder still has to read).  string: write_string."""
    if kind == "string":
        return write_string(x)
    if kind == "double" and isinstance(x, float):
        return _be(double_to_long_bits(bits_from_double(x)), 8)
    if kind == "float" and isinstance(x, float):
        return _be(float_to_int_bits_of_double(bits_from_double(x)), 4)
    if kind == "boolean" and isinstance(x, bool):
        x = int(x)
    return _be(x, SIZE[kind])


def frame(body):
    """SpanningRecordSerializer.addRecord: the length, then the bytes."""
    return _be(len(body), 4) + bytes(body)


def put_record(fields, values, ts=None):
    body = (b"\x00" + _be(ts, 8)) if ts is not None else b"\x01"
    return frame(body + b"".join(put_field(k, x) for (k, _), x in zip(fields, values)))


def put_watermark(wm):
    return frame(b"\x02" + _be(wm, 8))


def put_status(status):
    return frame(b"\x04" + _be(status, 4))


def put_latency(marked, id_lo, id_hi, subtask):
    return frame(b"\x03" + _be(marked, 8) + _be(id_lo, 8) + _be(id_hi, 8) + _be(subtask, 4))


# ---- reading --------------------------------------------------------------------------------------------------
def _read_varint(b, at, end):
    """-> (value mod 2^32, next position), or None when it runs past `end` or its fifth byte continues."""
    v, shift = 0, 0
    for k in range(5):
        if at + k >= end:
            return None
        c = b[at + k]
        v |= (c & 0x7f) << shift
        if c < 0x80:
            return v & 0xffffffff, at + k + 1
        shift += 7
    return None


def _read_string(b, at, end):
    """StringValue.readString (StringValue.java:745-787) -> (units or None for null, next), or None: past `end`."""
    r = _read_varint(b, at, end)
    if r is None:
        return None
    ln, at = r
    if ln == 0:
        return (None, at)
    units = []
    for _ in range(ln - 1):  # (runs out of bytes long before a corrupt, huge length is exhausted)
        r = _read_varint(b, at, end)
        if r is None:
            return None
        c, at = r
        units.append(c & 0xffff)  # (char) c
    return (units, at)


def string_hash_code(units):
    h = 0
    for c in units:
        h = (31 * h + c) & 0xffffffff
    return _signed(h, 32)


def string_key_id(units):
    """This build's 64-bit identity of a String key: FNV-1a 64 over the UTF-16 units, fmix64 of it ^ the length."""
    m = (1 << 64) - 1
    f = 0xcbf29ce484222325
    for c in units:
        f = ((f ^ c) * 0x100000001b3) & m
    x = f ^ len(units)
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & m
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & m
    x ^= x >> 33
    return _signed(x, 64)


def field_value(kind, b, at):
    """A fixed-size field as the operator's 64-bit column value (this build's choice, see the module docstring)."""
    if kind == "long" or kind == "double":
        return int.from_bytes(b[at:at + 8], "big", signed=True)
    if kind == "int":
        return int.from_bytes(b[at:at + 4], "big", signed=True)
    if kind == "short":
        return int.from_bytes(b[at:at + 2], "big", signed=True)
    if kind == "byte":
        return _signed(b[at], 8)
    if kind == "boolean":
        return int(b[at] != 0)
    if kind == "float":  # Float.intBitsToFloat, then the float's exact double (a NaN's payload is not pinned)
        return _signed(bits_from_double(struct.unpack(">f", b[at:at + 4])[0]), 64)
    raise ValueError(kind)


class Decoded:
    """key, key_hash, ts, val: the columns; stats: as the codec's; bad_pos / bad_tag: the corrupt element's byte
    position and code (None if the stream is clean); starts: where every accepted element begins."""

    def __init__(self, key, kh, ts, val, stats, bad_pos, bad_tag, starts):
        self.key = np.array(key, dtype=np.int64)
        self.key_hash = np.array(kh, dtype=np.int32)
        self.ts = np.array(ts, dtype=np.int64)
        self.val = np.array(val, dtype=np.int64)
        self.stats, self.bad_pos, self.bad_tag, self.starts = stats, bad_pos, bad_tag, starts


STRING_LIMIT = 64  # this build: a record with String fields is at most 64 bytes with its prefix


def decode(data, fields, string_limit=STRING_LIMIT):
    """The sequential walk of one channel's bytes: SpillingAdaptiveSpanningRecordDeserializer's role (a length, then
    that many bytes; a trailing partial element is left for the next call) around StreamElementSerializer.deserialize
    (StreamElementSerializer.java:199-221).  string_limit=None lifts this build's 64-byte limit on String records."""
    b = bytes(data)
    n = len(b)
    strings = any(k == "string" for k, _ in fields)
    F = sum(SIZE[k] for k, _ in fields if k != "string")
    kf = vf = None
    off = 0
    for k, r in fields:
        if k != "string":
            if r == "key":
                kf = (k, off)
            if r == "value":
                vf = (k, off)
            off += SIZE[k]
    key, kh, ts, val, starts = [], [], [], [], []
    st = dict(records=0, watermarks=0, latency_markers=0, statuses=0, consumed=0, watermark=LONG_MIN, status=0)
    pos, bad = 0, None
    from_bytes = int.from_bytes
    while pos + 4 <= n:
        ln = from_bytes(b[pos:pos + 4], "big")
        if pos + 4 + ln > n:
            break  # a partial element
        e = pos + 4
        if ln == 0:
            bad = -3  # readByte on an empty element: EOFException
            break
        tag = b[e] - 256 if b[e] >= 128 else b[e]  # source.readByte(): signed
        if tag < 0 or tag > 4:
            bad = tag
            break
        if tag <= 1:
            head = 9 if tag == 0 else 1
            p, end = e + head, e + ln
            if not strings:
                if ln != head + F:
                    bad = -2
                    break
                k = field_value(kf[0], b, p + kf[1]) if kf else 0
                v = field_value(vf[0], b, p + vf[1]) if vf else 0
                h = 0
            else:
                if string_limit is not None and 4 + ln > string_limit:
                    bad = -2
                    break
                k = v = h = 0
                null_key = False
                ok = ln >= head
                for kind, role in fields:
                    if not ok:
                        break
                    if kind == "string":
                        r = _read_string(b, p, end)
                        if r is None:
                            ok = False
                            break
                        units, p = r
                        if role == "key":
                            null_key = units is None
                            if units is not None:
                                k, h = string_key_id(units), string_hash_code(units)
                    else:
                        if p + SIZE[kind] > end:
                            ok = False
                            break
                        if role == "key":
                            k = field_value(kind, b, p)
                        if role == "value":
                            v = field_value(kind, b, p)
                        p += SIZE[kind]
                if not ok or p != end:
                    bad = -2
                    break
                if null_key:
                    bad = -4
                    break
            key.append(k)
            kh.append(h)
            val.append(v)
            ts.append(from_bytes(b[e + 1:e + 9], "big", signed=True) if tag == 0 else LONG_MIN)
            st["records"] += 1
        elif tag == 2:
            if ln != 9:
                bad = -2
                break
            st["watermarks"] += 1
            st["watermark"] = from_bytes(b[e + 1:e + 9], "big", signed=True)
        elif tag == 3:
            if ln != 29:
                bad = -2
                break
            st["latency_markers"] += 1
        else:
            if ln != 5:
                bad = -2
                break
            st["statuses"] += 1
            st["status"] = from_bytes(b[e + 1:e + 5], "big", signed=True)
        starts.append(pos)
        pos += 4 + ln
    st["consumed"] = pos
    return Decoded(key, kh, ts, val, st, pos if bad is not None else None, bad, starts)


# ---- encoding fired rows ----------------------------------------------------------------------------------------
def encode(rows, fields, f64=False):
    """rows: a mapping (or structured array) of the columns key / start / end / count / sum / min / max as 64-bit
    patterns (sum / min / max are double bits when f64).  One element per row: tag 0, timestamp
    window.maxTimestamp(), then the Tuple of the row fields the layout's roles name."""
    cols = {f: [int(x) for x in rows[f]] for f in ROW_FIELDS}
    out = bytearray()
    for r in range(len(cols["end"])):
        end = _signed(cols["end"][r], 64)
        # TimeWindow.java:83-85 `end - 1` (a Java long: Long.MIN_VALUE - 1 wraps to Long.MAX_VALUE); a count window's
        # row carries end = Long.MAX_VALUE for its GlobalWindow, whose maxTimestamp is Long.MAX_VALUE (:45-46)
        ts = LONG_MAX if end == LONG_MAX else _signed(end - 1, 64)
        body = bytearray(b"\x00" + _be(ts, 8))
        for kind, role in fields:
            v = cols[role][r] & ((1 << 64) - 1)
            dbl_field = kind in ("double", "float")
            dbl_value = bool(f64) and role in ("sum", "min", "max")
            if dbl_field:
                d = v if dbl_value else bits_from_double(float(_signed(v, 64)))  # (double) v: nearest even
                body += _be(double_to_long_bits(d), 8) if kind == "double" else _be(float_to_int_bits_of_double(d), 4)
            else:
                if dbl_value:
                    v = java_long_cast(v)
                body += _be(v, SIZE[kind])  # (int) / (short) / (byte): the low bytes
        out += frame(body)
    return bytes(out)
