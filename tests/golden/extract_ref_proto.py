"""Record the message / field names and field numbers the reference's wire schema declares, as data.

Run with the path of an eigen-zeth checkout:  python tests/golden/extract_ref_proto.py EIGEN_ZETH_DIR  -> tests/golden/ref_proto_schema.json

`proto/prover/v1/prover.proto` is the schema eigen-zeth's ProverChannel speaks (service ProverService, rpc ProverStream).
The output is DATA: for every message, the names of the fields it declares with their numbers (nested enums are not
fields), and the streaming shape of the one rpc; no text of the schema is stored.  tests/test_service.py pins the
product's mirror (eigen_zeth_amd/service/proto.py SCHEMA) on it."""
import json
import os
import re
import sys

SCHEMA = os.path.join("proto", "prover", "v1", "prover.proto")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_proto_schema.json")


def body_of(txt, name):
    m = re.search(r"message\s+%s\s*\{" % name, txt)
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(txt[i], 0)
        i += 1
    body = txt[m.end():i - 1]
    return re.sub(r"enum\s+\w+\s*\{.*?\}", "", body, flags=re.S)   # nested enums are not fields


def main(ref_root):
    txt = re.sub(r"//[^\n]*", "", open(os.path.join(ref_root, SCHEMA)).read())
    messages = {}
    for name in re.findall(r"message\s+(\w+)\s*\{", txt):
        messages[name] = {f: int(n) for f, n in re.findall(r"\b(\w+)\s*=\s*(\d+)\s*;", body_of(txt, name))}
    svc = re.search(r"service\s+(\w+)\s*\{", txt).group(1)
    rpc = re.search(r"rpc\s+(\w+)\s*\(\s*(stream\s+)?(\w+)\s*\)\s*returns\s*\(\s*(stream\s+)?(\w+)\s*\)", txt)
    out = {"source": "proto/prover/v1/prover.proto: declared fields (name -> number) per message; the service's rpc",
           "messages": messages,
           "rpc": {"service": svc, "method": rpc.group(1), "request": rpc.group(3), "request_stream": bool(rpc.group(2)),
                   "response": rpc.group(5), "response_stream": bool(rpc.group(4))}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
