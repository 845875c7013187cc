"""Pin the CompVis checkpoint key of every dump-tree tensor against the REFERENCE'S OWN Python side.
Needs a checkout of the reference; the fixture it writes is committed, so no test needs it.

    python tests/golden/gen_ckpt_keys.py <reference checkout>/python        # ~20 s, ~6 GB RAM, 4 GB of /tmp

python/dump.py's StableDiffusion is the object the reference fills with `load_state_dict(model, torch_load(ckpt)['state_dict'])`:
the dotted attribute path of every parameter IS its key in an SD v1.x checkpoint.  The reference's exporters
(python/stablediffusion.py: save_stable_diffusion) define the dump tree the engine's weight names come from.  Same method as
gen_from_reference_python.py, over the whole model:

 1. instantiate dump.StableDiffusion() through the tinygrad-API shim and walk it: {checkpoint key: tensor}.  Every tensor is
    filled with a unique constant; a 2-D tensor additionally gets a marker at [0, 1], which lands at flat index 1 of a dump
    that kept the layout and at flat index `rows` of one that holds the transpose (square Linear weights included);
 2. run save_stable_diffusion into a temporary tree;
 3. write tests/golden/sd14_ckpt_keys.txt, one line per dumped tensor:
        dump name <TAB> checkpoint key <TAB> checkpoint shape d0,d1,.. <TAB> T|-
    T: the dump holds the transpose of the checkpoint tensor (save.py:19, Linear weights).

tests/test_safetensors_cpu.py checks csrc/ckpt_keys.cpp against the fixture without the reference.
"""
import contextlib
import io
import shutil
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
OUT = HERE / "sd14_ckpt_keys.txt"
MARK = -7.0

import tinygrad_shim as shim  # noqa: E402


def walk(obj, prefix, out, seen):
    """{dotted attribute path: shim Tensor}: namedtuples by field, lists by index, dicts by key, objects by attribute."""
    if isinstance(obj, shim.Tensor):
        out[prefix] = obj
        return
    if id(obj) in seen:
        return
    seen.add(id(obj))
    dot = prefix + "." if prefix else ""
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        for f in obj._fields:
            walk(getattr(obj, f), dot + f, out, seen)
    elif isinstance(obj, (list, tuple)):
        for i, o in enumerate(obj):
            walk(o, dot + str(i), out, seen)
    elif isinstance(obj, dict):
        for k, o in obj.items():
            walk(o, dot + str(k), out, seen)
    elif hasattr(obj, "__dict__") and not isinstance(obj, (type, types.FunctionType, types.MethodType, types.ModuleType, types.BuiltinFunctionType)):
        for k, o in vars(obj).items():
            walk(o, dot + k, out, seen)


def main():
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    shim.DTYPE = torch.float32   # the constants are small integers: exact, and half the memory of the forward-pass generators
    shim.install()
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "dump.py").is_file():
        raise SystemExit("usage: gen_ckpt_keys.py <directory that holds the reference's dump.py, save.py, stablediffusion.py>")
    sys.path.insert(0, sys.argv[1])
    import dump                     # python/dump.py
    import stablediffusion as sd_save   # python/stablediffusion.py (exporter)

    model = dump.StableDiffusion()
    params = {}
    walk(model, "", params, set())
    by_index = {}
    for i, (key, p) in enumerate(params.items(), start=1):
        p.t = torch.full(tuple(p.t.shape), float(i), dtype=torch.float32)
        if p.t.ndim == 2 and p.t.shape[1] > 1:
            p.t[0, 1] = MARK
        by_index[i] = (key, p)
    print(f"python model: {len(params)} tensors ({time.time() - t0:.0f} s)", flush=True)

    tmp = Path(tempfile.mkdtemp(prefix="ckptkeys_"))
    lines = []
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            sd_save.save_stable_diffusion(model, tmp)
        print(f"reference exporters wrote the dump tree ({time.time() - t0:.0f} s)", flush=True)
        for f in sorted(tmp.rglob("*.npy")):
            name = str(f.relative_to(tmp))[:-4]
            if name.rsplit("/", 1)[-1] not in ("weight", "bias", "alphas_cumprod"):
                continue   # module metadata (eps, n_group, stride, n_head, n_steps ...): no checkpoint source
            raw = np.load(f, mmap_mode="r")
            for d in (1, 2, 4):   # save_tensor (save.py:10-15): the first D values are the shape; D is inferred
                dims = [int(v) for v in raw[:d]]
                if len(raw) == d + int(np.prod(dims)) and all(v > 0 for v in dims):
                    break
            else:
                raise RuntimeError(f"cannot parse {f}")
            key, p = by_index[int(raw[d])]
            shape = tuple(p.t.shape)
            transposed = False
            if d == 2 and shape[1] > 1:
                if raw[d + 1] == MARK:
                    assert shape == tuple(dims), (name, shape, dims)
                else:
                    assert raw[d + dims[1]] == MARK and shape == tuple(dims[::-1]), (name, shape, dims)
                    transposed = True
            else:
                assert shape == tuple(dims), (name, shape, dims)
            lines.append(f"{name}\t{key}\t{','.join(map(str, shape))}\t{'T' if transposed else '-'}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len({ln.split("\t")[1] for ln in lines}) == len(lines), "two dump files came from one checkpoint tensor"
    OUT.write_text("\n".join(lines) + "\n")
    print(f"wrote {OUT.name}: {len(lines)} dump tensors of {len(params)} checkpoint tensors ({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
