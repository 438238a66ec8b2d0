"""Every SF_* environment variable the library, the pipeline and bench.py read, with what it does (fifteen; the round-4 tree had seventy).  bench.py
refuses to run with an SF_* variable that is not in this table and prints the ones that are set in `config.switches` of its line; INTEGRATION.md
section 5 is generated from it (python -m slotformer_amd.switches).  Everything else that used to be an environment probe is either gone with the form
it selected (measured dead: profiles/r02..r05_probes.txt) or a keyword argument / command-line flag of the object it belongs to
(EncodeRolloutPipeline(...), bench.py --group / --cu-split / --partition / --steal / --force-dist ...).
PROCESS is the second table: every process-wide switch the library exports a setter and a getter for, whether it has a variable or not."""
import os

SWITCHES = {
    # ---- arithmetic and kernel forms (process defaults; per call: sf_rollout_opts / engine.rollout_opts) ----
    'SF_PRECISION': ('product', "process default of the matrix arithmetic: 'bf16x3' (default; split-bf16, fp32-equivalent) | 'f32' (exact-f32 MFMA) | 'bf16' (single pass)"),
    'SF_LAYER_TOK': ('product', "process default of sf_rollout_opts.layer_tok for DIRECT rollout calls (0, default: the row-tile / latency forms; 1: the layers before the last as token-stationary launches -- d_model 256 rollouters on the fused / long-window paths, and the OBJ3D shape (128, 8, 512) on the generic path, where it pays from ~64 videos per call and costs 7 % at 32: `sf_rollout_tok_layers` tells what a call takes). The pipeline passes its own choice per unit"),
    'SF_SEAM_FUSED': ('product', "process default of the seam launches of the latency forms (1; 0: two launches instead)"),
    'SF_CONV_FP16X2': ('product', "OPT-IN two-product fp16 form of the 5x5 convolutions (weights rounded to fp16: 3-6e-5 from the fixtures instead of 1e-5); default 0"),
    'SF_CONV_WS': ('product', "0: the 4-row-tile convolution everywhere (default 1: the weights-stationary kernel on streams with CUs of their own; the same bits)"),
    'SF_ENCODE_FORK': ('product', "direct encode calls as two branches on two streams (1, default) or one stream (0)"),
    # ---- the batch pipeline ----
    'SF_PIPE_TOK': ('product', "0: the pipeline never uses the token-stationary layer launches (every unit bit-identical to the serial module calls)"),
    'SF_PIPE_GROUP': ('product', "batches per rollout unit (default: 6 for token-stationary units of 32-video batches, else 4 / unit_batches_for)"),
    'SF_PIPE_HYBRID': ('product', "every k-th batch behind the fill is encoded on an unmasked stream beside the CU-masked lane (default 8 with token-stationary units, 3 / 5 / 0 otherwise)"),
    'SF_PIPE_FILL': ('product', "batches encoded on the whole chip at the start of a run (default: three units' worth)"),
    'SF_PIPE_CU_SPLIT': ('product', "CU mask of the encode partition, e.g. rows4 (default: sized from the two sides' CU time)"),
    'SF_PIPE_ENCODE_GRAPH': ('product', "replay the encode of a batch from a hipGraph (1, default) or launch it eagerly (0)"),
    # ---- tools ----
    'SF_PIPE_TRACE': ('tools', "record the device timeline of a run (tools/pipe_timeline.py)"),
    'SF_LIB_PATH': ('tools', "load another build of libslotformer_hip.so (tools/build_variant.sh: -D variants of a kernel)"),
    'SF_DBG': ('tools', "in-kernel time stamps and tuning overrides of the probes, comma separated: conv, lt, lf=<bits>, deconv, gemm, gemmcfg=<id>, convcfg=<id>, sab1 / flash1 (the packed-word attention backward / exact-f32 flash forward the bf16-plane kernels replaced), sabts (tools/*_probe.py)"),
}

# Every process-wide switch of libslotformer_hip.so (csrc/sf_switches.cpp holds the table the library reads): name -> (setter, getter, environment
# variable or None, default, what 1 / 0 select).  The environment variable is read once, on the first get, unless the setter was called before; a per-call
# option (sf_rollout_opts) wins over the process value for that call.  A switch is read when a call plans its launches: a hipGraph captured earlier keeps
# the form it was captured with.
PROCESS = {
    'precision': ('sf_set_precision', 'sf_get_precision', 'SF_PRECISION', 1, "matrix arithmetic: 0 exact-f32 MFMA, 1 split-bf16 (bf16x3), 2 single-pass bf16; the getter answers the calling thread's per-call precision while one is set"),
    'layer_tok': ('sf_set_layer_tok', 'sf_get_layer_tok', 'SF_LAYER_TOK', 0, "sf_rollout_opts.layer_tok == 0: the layers before the last of a rollout as token-stationary launches"),
    'seam_fused': ('sf_set_seam_fused', 'sf_get_seam_fused', 'SF_SEAM_FUSED', 1, "sf_rollout_opts.seam_fused == -1: seam launches of the rollout's latency forms"),
    'ffn_rows64': ('sf_set_ffn_rows64', 'sf_get_ffn_rows64', None, 0, "sf_rollout_opts.ffn_rows == 0: 64 instead of 32 rows per workgroup of the chunk-partial FFN launches (the same bits)"),
    'conv_fp16x2': ('sf_set_conv_fp16x2', 'sf_get_conv_fp16x2', 'SF_CONV_FP16X2', 0, "OPT-IN two-product fp16 arithmetic of the 64 -> 64 5x5 convolutions"),
    'slot_attn_tile16': ('sf_set_slot_attn_tile16', 'sf_get_slot_attn_tile16', None, 1, "9 .. 16 slots, keys == values: the one-pass tile kernel of Slot Attention (0: the two-pass kernel)"),
    'encode_fuse_next': ('sf_set_encode_fuse_next', 'sf_get_encode_fuse_next', None, 1, "the slot prologue of step t + 1 at the tail of step t's last slot update (0: its own launch; split-bf16 rounding apart)"),
    'slot_chain': ('sf_set_slot_chain', 'sf_get_slot_chain', None, 0, "OPT-IN: the slot branch of a batched encode as one video-stationary launch"),
    'slot_attn_planes': ('sf_set_slot_attn_planes', 'sf_get_slot_attn_planes', None, 1, "Slot-Attention iterations of the encode on feature rows kept as two bf16 planes, split-bf16 MFMAs (0: f32 rows, exact-f32 tile kernel)"),
    'pixel_tok': ('sf_set_pixel_tok', 'sf_get_pixel_tok', None, 1, "the per-pixel chain of the encoder in its pixel-stationary form (0: the tile kernels; another summation order)"),
}


def check_environment(environ=None):
    """(set, unknown): the SF_* variables of the environment that are in the table (name -> value), and the ones that are not."""
    environ = os.environ if environ is None else environ
    seen = {k: v for k, v in environ.items() if k.startswith('SF_')}
    return {k: v for k, v in seen.items() if k in SWITCHES}, sorted(k for k in seen if k not in SWITCHES)


def markdown_table():
    rows = ['| variable | kind | what it does |', '|---|---|---|']
    rows += [f'| `{k}` | {kind} | {text} |' for k, (kind, text) in SWITCHES.items()]
    return '\n'.join(rows)


def process_table():
    rows = ['| switch | setter / getter | environment | default | what it selects |', '|---|---|---|---|---|']
    rows += [f"| {k} | `{s}` / `{g}` | {f'`{env}`' if env else '-'} | {default} | {text} |" for k, (s, g, env, default, text) in PROCESS.items()]
    return '\n'.join(rows)


if __name__ == '__main__':
    print(markdown_table())
    print()
    print(process_table())
