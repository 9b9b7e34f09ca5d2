"""What lp_result_table_map must hold, derived from the oracle's records.

The oracle's record of a line is {"TYPE:path": [values]}: every delivery of a
path in delivery order, nulls included -- so a repeated name keeps ALL its
values, in order, under one key; what the record does not keep is the order
between different names.  The map of a wildcard "TYPE:prefix.*"
(ParsedRecord.setMultiValueString, ParsedRecord.java:185-196) follows from
it: the key is the path after "TYPE:prefix." (a member with an empty name is
delivered at "TYPE:prefix" itself: the key ""), a null neither adds nor
replaces, the last non-null value wins.  The entry ORDER the project fixes (a
surviving entry stands at its last delivery) is not in the record: the tests
check it on hand-written lines, and device against host byte for byte.
"""
import json


def as_string(v):
    """Value.getString of a record value: a string, or {"l": n} for a long"""
    return str(v["l"]) if isinstance(v, dict) else v


def expected_map(record, path):
    """the map of wildcard `path` ("TYPE:prefix.*") for one oracle record"""
    assert path.endswith(".*"), path
    exact = path[:-2]
    pre = exact + "."
    out = {}
    for k, vals in record.items():
        if k == exact:
            key = ""
        elif k.startswith(pre):
            key = k[len(pre):]
        else:
            continue
        live = [v for v in vals if v is not None]
        if live:
            out[key] = as_string(live[-1])
    return out


def deliveries(record, path):
    """how many values (nulls included) the record holds under the wildcard"""
    exact = path[:-2]
    return sum(len(v) for k, v in record.items() if k == exact or k.startswith(exact + "."))


_REF = {}  # (key, paths) -> per line [maps per path] or None: computed once, never changed


def oracle_maps(oracle, key, fmt, fields, lines, paths, remaps=()):
    """per line: None when the oracle's line is not OK, else {path: map}.
    The oracle parser is stateful (sticky LogFormat): every line, in order."""
    k = (key, fmt, tuple(fields), len(lines), tuple(paths), tuple(remaps))
    if k not in _REF:
        o = oracle.Oracle(fmt, list(fields), list(remaps))
        out = []
        for l in lines:
            st, js = o.parse_raw(l)
            if st != oracle.OK:
                out.append(None)
                continue
            rec = json.loads(js)
            out.append({p: expected_map(rec, p) for p in paths} | {"#deliveries": {p: deliveries(rec, p) for p in paths}})
        _REF[k] = out
    return _REF[k]
