#!/usr/bin/env python3
"""Dump what the host side of the library plans for a fixed list of configs of the three families (no GPU)."""
import ctypes as C
import hashlib
import json
import os
import sys

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else ".")
from ishara_amd import _lib, make_config                      # noqa: E402
from ishara_amd.model import Model                            # noqa: E402
from ishara_amd.conformer import ConformerEncoder             # noqa: E402
from ishara_amd.squeezeformer import SqueezeformerEncoder     # noqa: E402

KERAS = [dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=1, dtype="f32"),
         dict(dim=256, input_shape=(384, 224), max_batch=256),
         dict(dim=256, input_shape=(384, 276), max_batch=1, dtype="f16"),
         dict(dim=256, num_conv_squeeze_blocks=4, num_conv_conform_blocks=4, num_conv_per_block=0, squeeze_expansion=4, conformer_expansion=2, top_dim=256, max_batch=2),
         dict(dim=512, num_conv_squeeze_blocks=6, num_conv_conform_blocks=6, input_shape=(512, 224), max_batch=8)]
CONF = [dict(dim=64, num_layers=2, num_heads=4, expansion_factor=2, kernel_size=7, seq_len=48, max_batch=2, dtype="f32"),
        dict(dim=256, num_layers=7, seq_len=384, max_batch=16, dtype="bf16")]
SQZ = [dict(input_dim=40, encoder_dim=64, num_layers=4, reduce_layer_index=1, recover_layer_index=3, num_attention_heads=4, conv_kernel_size=7, seq_len=64, max_batch=2, dtype="f32"),
       dict(input_dim=80, encoder_dim=256, num_layers=16, reduce_layer_index=7, recover_layer_index=15, seq_len=384, max_batch=4, dtype="bf16"),
       dict(input_dim=80, encoder_dim=128, num_layers=3, reduce_layer_index=9, recover_layer_index=9, num_attention_heads=4, seq_len=128, max_batch=2, dtype="bf16")]


def plan(obj):
    lib, h = obj._lib, obj._h
    ent = hashlib.sha256(json.dumps(obj.entries).encode()).hexdigest()[:16]
    buckets = []
    for i in range(lib.ishara_grad_buckets(h)):
        o, c = C.c_int64(), C.c_int64()
        lib.ishara_grad_bucket(h, i, C.byref(o), C.byref(c))
        buckets.append((o.value, c.value))
    return dict(n_entries=len(obj.entries), entries_sha=ent, n_total=obj.n_total, n_train=obj.n_train,
                workspace_bytes=int(lib.ishara_workspace_bytes(h)), plan_buffers=int(lib.ishara_workspace_plan_check(h)), buckets=buckets,
                out_frames=int(lib.ishara_encoder_output_frames(h)))


out = {}
for guard in ("0", "1"):
    os.environ["ISHARA_WS_GUARD"] = guard
    for i, kw in enumerate(KERAS):
        out[f"keras{i}/guard{guard}"] = plan(Model(make_config(**kw), device=None))
    for i, kw in enumerate(CONF):
        out[f"conformer{i}/guard{guard}"] = plan(ConformerEncoder(**kw, device=None))
    for i, kw in enumerate(SQZ):
        out[f"squeezeformer{i}/guard{guard}"] = plan(SqueezeformerEncoder(**kw, device=None))
print(json.dumps(out, indent=1, sort_keys=True))
