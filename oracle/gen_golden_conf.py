"""Golden record of the reference's shipped configs, read with this repository's own loader (fs_eend_amd.config).

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_conf.py <reference project root>

Every `<root>/*/conf/*.yaml` is loaded with `config.load` (the `!ref` references resolved); the record keeps, per file,
its top-level sections, and for the two configs this repository mirrors (fs-eend_amd/conf/*_simu.yaml) the values the
tests compare: model.params, the data keys of the feature geometry and the optimiser keys of `training`.  Only parsed
values are stored (tests/golden/reference_configs.json), no config text.
"""
import glob
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from fs_eend_amd import config as CFG  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_configs.json")
FS_CONF = "FS-EEND/conf/spk_onl_tfm_enc_dec_nonautoreg.yaml"
LS_CONF = "LS-EEND/conf/spk_onl_conformer_retention_enc_dec_nonautoreg.yaml"
DATA_KEYS = ("max_speakers", "context_recp", "chunk_size", "subsampling", "label_delay", "feat_type")
TRAIN_KEYS = ("lr", "grad_clip", "warm_steps", "schedule_scale", "batch_size")


def main(ref):
    configs = {}
    for path in sorted(glob.glob(os.path.join(ref, "*", "conf", "*.yaml"))):
        cfg = CFG.load(path)
        assert isinstance(cfg, dict) and "model" in cfg, path
        configs[os.path.relpath(path, ref)] = dict(sections=sorted(cfg))
    fs, ls = CFG.load(os.path.join(ref, FS_CONF)), CFG.load(os.path.join(ref, LS_CONF))
    rec = dict(configs=configs,
               fs=dict(file=FS_CONF, model_params=fs["model"]["params"], data={k: fs["data"][k] for k in DATA_KEYS},
                       training={k: fs["training"][k] for k in TRAIN_KEYS}),
               ls=dict(file=LS_CONF, model_params=ls["model"]["params"]))
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(configs)} configs -> {os.path.relpath(OUT)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
