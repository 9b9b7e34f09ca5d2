"""An independent Python restatement of the two dissectors that work on a
type-remapped value, for the tests' expectations (the oracle has neither):

  ScreenResolutionDissector.dissect (hp/dissectors/ScreenResolutionDissector.java:48-65)
  ModUniqueIdDissector.decode       (hp/dissectors/ModUniqueIdDissector.java:149-238)

Applied to the source value the corpus generator planted (after URL decoding,
for a query parameter)."""
import base64
import struct

ID_ALPHABET = frozenset("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_")


def java_parse_long(s):
    """Value.getLong of a string (core/Value.java:59-66): Long.parseLong, None on failure"""
    if s is None or s == "":
        return None
    body = s[1:] if s[0] in "+-" else s
    if not body or not all("0" <= ch <= "9" for ch in body):
        return None
    v = int(body)
    v = -v if s[0] == "-" else v
    return v if -(1 << 63) <= v < (1 << 63) else None


def screen(v, want_w, want_h):
    """{"width": str, "height": str} of the requested outputs for source value
    v (None: no value); {} when nothing is delivered.  IndexError where the
    reference throws ArrayIndexOutOfBoundsException: the line is FALLBACK."""
    if v is None or v == "" or "x" not in v:
        return {}
    parts = v.split("x")
    while parts and parts[-1] == "":  # String.split drops trailing empty strings only
        parts.pop()
    out = {}
    if want_w:
        out["width"] = parts[0]
    if want_h:
        out["height"] = parts[1]
    return out


def unique_id(v):
    """{"epoch", "ip", "processid", "counter", "threadindex"} of source value v, {} when
    nothing is delivered: anything but exactly 24 letters of [A-Za-z0-9_-]"""
    if v is None or len(v.encode("utf-8")) != 24 or not all(ch in ID_ALPHABET for ch in v):
        return {}
    b = base64.b64decode(v, altchars=b"-_")
    assert len(b) == 18
    t, ip, pid, ctr, thr = struct.unpack(">IIIHI", b)
    return {"epoch": t * 1000, "ip": ".".join(str(x) for x in struct.pack(">I", ip)), "processid": pid, "counter": ctr,
            "threadindex": thr}
