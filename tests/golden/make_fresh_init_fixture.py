#!/usr/bin/env python3
"""SHA-256 of the tensors ``from_pretrained`` leaves freshly initialised (PyTorch-default init, generator seed 0) for the tiny UNet and
the tiny prior of tests/test_from_pretrained.py, on directories that hold a ``config.json`` and no checkpoint: every tensor is fresh.

The initialisation draws from one generator in the iteration order of ``expected_shapes()``; anything that reorders the draws or changes
a bound changes every later tensor.  tests/test_from_pretrained.py::test_fresh_init_matches_the_recorded_values holds the code to these
values, so the fixture is generated ONCE, by the commit before a change to the init code, never by the code under test.

    python tests/golden/make_fresh_init_fixture.py
writes tests/golden/fresh_init_sha256.json.
"""
from __future__ import annotations

import hashlib
import json
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

UNET_KW = dict(subfolder="unet", in_channels=9, class_embed_type="projection", projection_class_embeddings_input_dim=64,
               ignore_mismatched_sizes=True)
PRIOR_JSON = {"_class_name": "PriorTransformer", "num_attention_heads": 2, "attention_head_dim": 64, "num_layers": 2,
              "embedding_dim": 1280, "num_embeddings": 77, "additional_embeddings": 4, "dropout": 0.0}
PRIOR_KW = dict(subfolder="prior", num_embeddings=2, embedding_dim=1024, ignore_mismatched_sizes=True)
NAMED = {"unet": ("conv_in.weight", "conv_in.bias", "class_embedding.linear_1.weight", "class_embedding.linear_2.bias",
                  "mid_block.resnets.0.conv1.weight", "conv_out.weight"),
         "prior": ("pose_encoder.net.0.weight", "pose_encoder1.net.4.bias", "proj_in.weight", "positional_embedding", "prd_embedding",
                   "transformer_blocks.1.ff.net.2.weight", "proj_to_clip_embeddings.weight")}


def sha(t: torch.Tensor) -> str:
    assert t.dtype == torch.float32
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def digest(sd, named) -> dict:
    """``all``: one hash over (name, shape, bytes) of every tensor in the state dict's order; plus the hash of each tensor of ``named``."""
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(f"{k}{tuple(v.shape)}".encode())
        h.update(v.contiguous().numpy().tobytes())
    return {"all": h.hexdigest(), "count": len(sd), **{k: sha(sd[k]) for k in named}}


def fresh_models(tmp: Path):
    """(name, model) of the two config-only ``from_pretrained`` calls."""
    import pcdms_amd as P
    from tests.test_from_pretrained import SD21_UNET_JSON
    for sub, cfg in (("unet", SD21_UNET_JSON), ("prior", PRIOR_JSON)):
        (tmp / sub).mkdir(parents=True, exist_ok=True)
        (tmp / sub / "config.json").write_text(json.dumps(cfg))
    yield "unet", P.Stage2_InapintUNet2DConditionModel.from_pretrained(tmp, **UNET_KW)
    yield "prior", P.Stage1_PriorTransformer.from_pretrained(tmp, **PRIOR_KW)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = {name: digest(m.state_dict(), NAMED[name]) for name, m in fresh_models(Path(tmp))}
    out["torch_version"] = torch.__version__
    path = ROOT / "tests" / "golden" / "fresh_init_sha256.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
