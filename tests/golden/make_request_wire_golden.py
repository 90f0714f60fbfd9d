#!/usr/bin/env python3
"""Generate tests/golden/request_wire_cases.json.

Two things, data only:

``schema``: the field tables of ConfChange, ConfChangeSingle and ConfChangeV2
read out of the reference's own FileDescriptorProto (raft/raftpb/raft.pb.go:698)
with the oracle's restated wire decoder, exactly as make_raftpb_schema.py does
for Message, and cross-checked against Google's protobuf runtime parsing the
same bytes.  tests/request_wire_ref.py's CC_SCHEMAS is pinned to them.

``cases``: the conf changes the reference's tests propose, transcribed as field
values, each with the wantsLeaveJoint that raft.go:1053 yields for it
(len(cc.AsV2().Changes) == 0; AsV2 of a V1 has one change, confchange.go:63-73):
rawnode_test.go TestRawNodeProposeAndConfChange (V1 and V2, implicit and
explicit joint, the V2 that leaves manually and the empty one that leaves
automatically) and raft_test.go TestStepConfig, TestStepIgnoreConfig and
TestProposalByProxy.

    python tests/golden/make_request_wire_golden.py [/root/reference]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import raftpb_ref as r  # noqa: E402
import make_raftpb_schema as S  # noqa: E402

KINDS = ("ConfChange", "ConfChangeSingle", "ConfChangeV2")
ADD_NODE, REMOVE_NODE, UPDATE_NODE, ADD_LEARNER = 0, 1, 2, 3  # ConfChangeType (raft.pb.go:224-227)
AUTO, IMPLICIT, EXPLICIT = 0, 1, 2                            # ConfChangeTransition (raft.pb.go:171-183)
ENTRY_NORMAL, ENTRY_CONF_CHANGE, ENTRY_CONF_CHANGE_V2 = 0, 1, 2
THREE = [[ADD_NODE, 2], [ADD_LEARNER, 1], [ADD_LEARNER, 3]]
RAWNODE = "rawnode_test.go TestRawNodeProposeAndConfChange"


def v1(source, ctype, node, data_nil=False):
    return {"source": source, "entry_type": ENTRY_CONF_CHANGE, "data_nil": data_nil,
            "v1": {"id": 0, "type": ctype, "node_id": node, "context": None},
            "wants_leave_joint": False}


def v2(source, changes, transition=AUTO, context=None):
    return {"source": source, "entry_type": ENTRY_CONF_CHANGE_V2, "data_nil": False,
            "v2": {"transition": transition, "changes": changes, "context": context},
            "wants_leave_joint": len(changes) == 0}


CASES = [
    v1(RAWNODE + " case 1 (V1)", ADD_NODE, 2),
    v2(RAWNODE + " case 2 (V2, simple)", [[ADD_NODE, 2]]),
    v2(RAWNODE + " case 3 (learner)", [[ADD_LEARNER, 2]]),
    v2(RAWNODE + " case 4 (explicit joint)", [[ADD_LEARNER, 2]], EXPLICIT),
    v2(RAWNODE + " case 5 (implicit joint)", [[ADD_LEARNER, 2]], IMPLICIT),
    v2(RAWNODE + " case 6 (three changes, auto)", THREE),
    v2(RAWNODE + " case 7 (three changes, explicit)", THREE, EXPLICIT),
    v2(RAWNODE + " case 8 (three changes, implicit)", THREE, IMPLICIT),
    v2(RAWNODE + " leaving manually: ConfChangeV2{Context: manual}", [], AUTO, "manual"),
    v2(RAWNODE + " leaving automatically: the zero ConfChangeV2", []),
    # Entries: []pb.Entry{{Type: pb.EntryConfChange}}: nil Data, the zero ConfChange
    v1("raft_test.go TestStepConfig", ADD_NODE, 0, data_nil=True),
    v1("raft_test.go TestStepIgnoreConfig (both proposals)", ADD_NODE, 0, data_nil=True),
    # Entries: []pb.Entry{{Data: []byte("somedata")}}: a normal entry, no conf change
    {"source": "raft_test.go TestProposalByProxy", "entry_type": ENTRY_NORMAL, "data_nil": False,
     "data": "somedata", "wants_leave_joint": None},
]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    fdp = S.reference_descriptor(ref)
    f = r.descriptor_fields(fdp)
    schema = {k: {str(n): f[k][n] for n in sorted(f[k])} for k in KINDS}
    from google.protobuf import descriptor_pb2
    fd = descriptor_pb2.FileDescriptorProto()
    fd.ParseFromString(fdp)
    byname = {m.name: m for m in fd.message_type}
    for k in KINDS:
        got = {str(x.number): (x.name, x.type, x.label, x.type_name) for x in byname[k].field}
        want = {n: (v["name"], v["type"], v["label"], v["type_name"]) for n, v in schema[k].items()}
        assert got == want, (k, got, want)
    out = {"source": f"raft/raftpb/raft.pb.go:698 ({S.VAR}, gzipped FileDescriptorProto, "
                     f"{len(fdp)} bytes decoded); the cases: raft/rawnode_test.go:114-374, "
                     "raft/raft_test.go (TestStepConfig, TestStepIgnoreConfig, TestProposalByProxy)",
           "schema": schema, "cases": CASES}
    path = os.path.join(ROOT, "tests", "golden", "request_wire_cases.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
