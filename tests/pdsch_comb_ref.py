"""numpy statement of the rule that combines the redundancy versions of one SI transport block (include/lcs.h: lcs_pdsch_comb_info), on
top of tests/pdsch_ref.py and written from the rule's text, not from the product's header: the reference of every test of that stage.
It takes pdsch_ref.receive's blocks (which carry their soft bits) and gives the groups with their summed streams."""
import numpy as np

import pdsch_ref as SR

STATUS = dict(member=1, ok=2, crc=3, silent=4)
MAX_GROUPS, MAX_MEMBERS = 8, 4


def is_member(b):
    return b["kind"] == 1 and b["status"] in (SR.STATUS["ok"], SR.STATUS["crc"])


def grouping(blocks, si_window=0, sib1=True):
    """-> list of (rule, [block indices]) in the order of their first member, every group there is"""
    groups = []          # dict(rule, key, first_sf, members)
    for i, b in enumerate(blocks[:32]):
        if not is_member(b):
            continue
        if sib1 and b["subframe"] % 10 == 5:
            rule, key = 1, (b["tbs"], (b["subframe"] // 10) % 2)
        elif si_window > 0:
            rule, key = 2, (b["tbs"],)
        else:
            continue
        mine = [g for g in groups if g["rule"] == rule and g["key"] == key]
        g = mine[-1] if mine else None
        if g is not None and (len(g["members"]) >= MAX_MEMBERS or (rule == 2 and b["subframe"] - g["first_sf"] >= si_window)):
            g = None
        if g is None:
            g = dict(rule=rule, key=key, first_sf=b["subframe"], members=[])
            groups.append(g)
        g["members"].append(i)
    return [(g["rule"], g["members"]) for g in groups]


def summed(blocks, members):
    """d [3][K + 4]: 0 + the members' de-rate-matched values in ascending member order"""
    b0 = blocks[members[0]]
    d = np.zeros((3, b0["K"] + 4))
    for i in members:
        b = blocks[i]
        assert (b["K"], b["F"]) == (b0["K"], b0["F"])
        d = d + SR.derm(b["llr"], b["K"], b["F"], b["rv"])
    return d


def combine(blocks, si_window=0, sib1=True, max_iter=8):
    """-> dict(groups: the listed groups as dicts (members, rule, tbs, K, F, rv_mask, n_ok_members, n_same, n_iter, status, payload [280],
    margin, d: the summed streams of a decoded group or None), n_overflow)"""
    out = []
    all_groups = grouping(blocks, si_window, sib1)
    for rule, members in all_groups[:MAX_GROUPS]:
        mb = [blocks[i] for i in members]
        ok = [b for b in mb if b["status"] == SR.STATUS["ok"]]
        g = dict(members=members, rule=rule, tbs=mb[0]["tbs"], K=mb[0]["K"], F=mb[0]["F"], rv_mask=int(np.bitwise_or.reduce([1 << b["rv"] for b in mb])),
                 n_ok_members=len(ok), n_same=0, n_iter=0, payload=np.zeros(280, np.uint8), margin=np.inf, d=None)
        if ok:
            g.update(status=STATUS["member"], payload=ok[0]["payload"], n_same=sum(np.array_equal(b["payload"], ok[0]["payload"]) for b in ok))
        elif len(mb) == 1:
            g.update(status=STATUS["crc"], payload=mb[0]["payload"])
        else:
            with np.errstate(all="ignore"):
                d = summed(blocks, members)
            res = SR.turbo_decode(d, g["K"], g["F"], max_iter)
            st = {SR.STATUS["ok"]: STATUS["ok"], SR.STATUS["crc"]: STATUS["crc"], SR.STATUS["silent"]: STATUS["silent"]}[res["status"]]
            g.update(status=st, n_iter=res["n_iter"], margin=res["margin"], d=d)
            if st != STATUS["silent"]:
                g["payload"] = SR.payload_bytes(res["bits"], g["F"], g["tbs"])
        out.append(g)
    return dict(groups=out, n_overflow=max(0, len(all_groups) - MAX_GROUPS))
