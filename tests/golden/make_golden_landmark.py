"""Writes tests/golden/landmark_2d106det.npz: what the reference's symbol file says about the 106-point landmark
network, as data, plus the float64 restatement's outputs.

    python tests/golden/make_golden_landmark.py [<reference tree>]

From coordinate_reg/model/2d106det-symbol.json (read when the reference tree is given; without it the graph records
of the existing fixture are kept):
  param_names / param_kinds / param_shapes   every parameter node in graph order, 'arg' or 'aux' (an input of a
                                             BatchNorm at position 3 or 4), its shape inferred by walking the graph
  layer_names / layer_ops / layer_attrs      every operator node: op and, for a Convolution, kernel, stride, pad,
                                             groups, filters; for fc1, num_hidden; the two input scalars
The maker asserts that ghost_amd.landmarks' own table equals these records.

From tests/landmark_ref.py (float64, N = 2, the key-hashed weights): pred and the four taps.  They pin the
restatement against drift; they are not a reference run (mxnet is not installed and no checkpoint is available:
numerics against mxnet are unpinned).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "landmark_2d106det.npz")
GRAPH_KEYS = ["param_names", "param_kinds", "param_shapes", "layer_names", "layer_ops", "layer_attrs", "in_scalars"]


def _tup(s):
    return tuple(int(v) for v in s.strip("()").split(",") if v.strip())


def read_symbol(path):
    with open(path) as f:
        nodes = json.load(f)["nodes"]
    aux = set()
    for n in nodes:
        if n["op"] == "BatchNorm":
            aux.update(nodes[i[0]]["name"] for i in n["inputs"][3:5])
    shapes, shape_of = {}, {}         # parameter name -> shape; node index -> (C, H, W) of its output
    layer_names, layer_ops, layer_attrs, scalars = [], [], [], []
    for idx, n in enumerate(nodes):
        op, a = n["op"], n.get("attrs", {})
        ins = [i[0] for i in n["inputs"]]
        if op == "null":
            if n["name"] == "data":
                shape_of[idx] = (3, 192, 192)
            continue
        c, h, w = shape_of[ins[0]]
        attrs = [0, 0, 0, 0, 0]       # kernel, stride, pad, groups, filters
        if op in ("_minus_scalar", "_mul_scalar"):
            scalars.append(float(a["scalar"]))
        elif op == "Convolution":
            assert a["no_bias"] == "True" and len(ins) == 2
            k, s, p = _tup(a["kernel"]), _tup(a["stride"]), _tup(a["pad"])
            g, f = int(a["num_group"]), int(a["num_filter"])
            assert k[0] == k[1] and s[0] == s[1] and p[0] == p[1]
            attrs = [k[0], s[0], p[0], g, f]
            shapes[nodes[ins[1]]["name"]] = (f, c // g, k[0], k[1])
            c, h, w = f, (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[0] - k[0]) // s[0] + 1
        elif op == "BatchNorm":
            assert a == {"fix_gamma": "True"}          # no eps, no momentum: mxnet's defaults
            for i in ins[1:]:
                shapes[nodes[i]["name"]] = (c,)
        elif op == "LeakyReLU":
            assert a == {"act_type": "prelu"}
            shapes[nodes[ins[1]]["name"]] = (c,)
        elif op == "Flatten":
            c, h, w = c * h * w, 1, 1
        elif op == "FullyConnected":
            nh = int(a["num_hidden"])
            attrs[4] = nh
            shapes[nodes[ins[1]]["name"]] = (nh, c)
            shapes[nodes[ins[2]]["name"]] = (nh,)
            c = nh
        else:
            raise SystemExit(f"unexpected op {op}")
        shape_of[idx] = (c, h, w)
        layer_names.append(n["name"])
        layer_ops.append(op)
        layer_attrs.append(attrs)
    names = [n["name"] for n in nodes if n["op"] == "null" and n["name"] != "data"]
    pad = lambda s: list(s) + [0] * (4 - len(s))
    return {"param_names": np.array(names), "param_kinds": np.array(["aux" if n in aux else "arg" for n in names]),
            "param_shapes": np.array([pad(shapes[n]) for n in names], np.int32), "layer_names": np.array(layer_names),
            "layer_ops": np.array(layer_ops), "layer_attrs": np.array(layer_attrs, np.int32),
            "in_scalars": np.array(scalars)}


def own_graph():
    """The same records from ghost_amd.landmarks.pack's table."""
    from ghost_amd.landmarks import pack
    specs = pack.param_specs()
    names, ops, attrs = ["_minusscalar0", "_mulscalar0"], ["_minus_scalar", "_mul_scalar"], [[0] * 5, [0] * 5]
    for pre, _ci, co, k, s, p, g in pack.conv_layers():
        names += [f"{pre}_conv2d", f"{pre}_batchnorm", f"{pre}_relu"]
        ops += ["Convolution", "BatchNorm", "LeakyReLU"]
        attrs += [[k, s, p, g, co], [0] * 5, [0] * 5]
    names += ["flatten0", "fc1"]
    ops += ["Flatten", "FullyConnected"]
    attrs += [[0] * 5, [0, 0, 0, 0, 2 * pack.N_POINTS]]
    pad = lambda s: list(s) + [0] * (4 - len(s))
    return {"param_names": np.array([n for n, _, _ in specs]), "param_kinds": np.array([k for _, _, k in specs]),
            "param_shapes": np.array([pad(s) for _, s, _ in specs], np.int32), "layer_names": np.array(names),
            "layer_ops": np.array(ops), "layer_attrs": np.array(attrs, np.int32),
            "in_scalars": np.array(pack.IN_SCALARS)}


def main():
    import torch

    import landmark_ref
    if len(sys.argv) > 1:
        graph = read_symbol(os.path.join(sys.argv[1], "coordinate_reg", "model", "2d106det-symbol.json"))
    else:
        with np.load(OUT) as z:
            graph = {k: z[k] for k in GRAPH_KEYS}
    own = own_graph()
    for k in GRAPH_KEYS:
        assert graph[k].shape == own[k].shape and bool((graph[k] == own[k]).all()), f"{k} differs from the symbol file"
    p = landmark_ref.make_weights()
    pred, taps = landmark_ref.forward(p, landmark_ref.make_input(2), bgr=True, dtype=torch.float64)
    out = dict(graph)
    out["pred"] = pred.numpy()
    # the taps as float32, conv_2 (2 x 32 x 96 x 96 values) at every fourth row and column: enough to pin a float64
    # restatement to 1e-6 within the size a committed file may have
    for n, t in taps.items():
        out[f"tap_{n}"] = (t[:, :, ::4, ::4] if n == "conv_2" else t).numpy().astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
