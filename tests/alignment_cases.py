"""The pointer-alignment table of the C ABI (a helper, not a test; plain data plus the code that turns a row into a call).

One rule (include/xpretrain_hip.h, "Pointer alignment"): every device pointer an entry receives has ONE class per (entry, operand):

  ``need N``     a base that is not N-byte aligned is refused on the host before anything is launched; xp_last_error() names the
                 entry, the operand and N.  ``need 8/16`` is N = 8 with bf16 storage and 16 with fp32 (four elements per access).
  ``any``        every element-aligned base is served: the kernels behind that operand read and write it one element at a time, or
                 take a wider path only where the address allows it.

``ROWS`` holds one row per (entry, operand), ``EXEMPT`` every pointer parameter or structure field that is no device operand,
with the reason.  ``CALLS`` holds the smallest valid call of every entry that takes a
device pointer: the scalar arguments by header name (pointer operands get addresses from the test: synthetic ones on a machine
without a GPU, guarded buffers on one with).  tests/test_alignment_cpu.py holds this table against the header (every pointer
parameter and structure field is here; the header's ``align[...]`` comments say the same) and makes every refusal;
tests/test_alignment_gpu.py runs the ``any`` rows misaligned and the refusals over real buffers."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xpretrain_hip.h")
BF16, F32 = 0, 1

# ------------------------------------------------------------------------------------------------------------ the header, as text
_PROTO = re.compile(r"([^;(){}#]+?)\b(xp_\w+)\s*\(([^;(){}#]*)\)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FIELD = re.compile(r"(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?$")


def _header_text():
    with open(HEADER) as f:
        return f.read()


def prototypes(text=None):
    """{entry: [(C type without the name, parameter name, is a pointer)]} in header order"""
    text = re.sub(r"/\*.*?\*/", " ", text if text is not None else _header_text(), flags=re.S)
    out = {}
    for m in _PROTO.finditer(text):
        params = []
        for p in ([] if m[3].strip() in ("", "void") else m[3].split(",")):
            p = " ".join(p.split())
            name = re.search(r"(\w+)$", p)[1]
            params.append((p[:-len(name)].strip(), name, "*" in p))
        out[m[2]] = params
    return out


def struct_fields(text=None):
    """{struct: [(base C type, field name, is a pointer, array length or 0)]}"""
    text = re.sub(r"/\*.*?\*/", " ", text if text is not None else _header_text(), flags=re.S)
    out = {}
    for m in _STRUCT.finditer(text):
        fields = []
        for decl in m[1].split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            first, *more = [d.strip() for d in decl.split(",")]
            f = _FIELD.match(first)
            base, stars, name, n = f.groups()
            fields.append((base, name, bool(stars), int(n or 0)))
            for extra in more:
                g = re.match(r"(\w+)\s*(?:\[\s*(\d+)\s*\])?$", extra)
                fields.append((base, g[1], False, int(g[2] or 0)))
        out[m[2]] = fields
    return out


def header_classes(text=None):
    """the header's own statement: {entry: {operand: class}} from its ``align[entry]: class: a b; class: c`` comments.
    ``all need 16`` (or ``all`` of another class) stands for every operand the comment does not name."""
    text = text if text is not None else _header_text()
    out = {}
    for m in re.finditer(r"align\[(\w+)\]:([^*]*?)\*/", text):
        entry, body = m[1], " ".join(m[2].split())
        assert entry not in out, f"two align[] comments for {entry}"
        rows = {}
        for part in [p.strip() for p in body.split(";") if p.strip()]:
            if part.startswith("all "):
                rows["*"] = part[4:].strip()
                continue
            cls, names = part.split(":")
            for n in names.split():
                assert n not in rows, (entry, n)
                rows[n] = cls.strip()
        out[entry] = rows
    return out


# ------------------------------------------------------------------------------------------------------------ what is no operand
# by parameter name, in every entry
EXEMPT_NAMES = {
    "stream": "a hipStream_t handle, not memory",
    "mean3_host": "host array (copied into the kernel-argument block)",
    "std3_host": "host array (copied into the kernel-argument block)",
    "group_of_host": "host array (copied into the kernel-argument block)",
    "groups_host": "host array (copied into the kernel-argument block)",
}
# (entry, parameter): host structures the call reads, host out-parameters of planning and sizing queries, debug entries
EXEMPT = {
    ("xp_gemm_auto_split", "desc"): "planning query over a host struct: the data pointers are ignored",
    ("xp_gemm_auto_split_slack", "desc"): "planning query over a host struct: the data pointers are ignored",
    ("xp_gemm_colsum_rows", "desc"): "planning query over a host struct: the data pointers are ignored",
    ("xp_gemm_tile_rows", "desc"): "planning query over a host struct: the data pointers are ignored",
    ("xp_debug_gemm_plan", "desc"): "planning query over a host struct: the data pointers are read as present / absent",
    ("xp_debug_gemm_plan", "out"): "host out-parameter of a planning query",
    ("xp_debug_attn_plan", "out"): "host out-parameter of a planning query",
    ("xp_debug_attn_pooled_plan", "out"): "host out-parameter of a planning query",
    ("xp_debug_layer_bwd_gemms", "dims"): "host struct without pointers",
    ("xp_debug_layer_bwd_gemms", "out"): "host out-parameter: descriptors without operands",
    ("xp_debug_gemm_timer_read", "ms"): "host out-parameter of a debug entry",
    ("xp_reduce_rows_batch_workspace_bytes", "segs_host"): "sizing query over a host array: reads the widths only",
    ("xp_frames_transform_aa_workspace_bytes", "videos_host"): "sizing query over a host array: no pointer is dereferenced",
    ("xp_retrieval_stream_plan", "stat_tiles_per_split"): "host out-parameter of a planning query",
    ("xp_retrieval_stream_plan", "topk_tiles_per_split"): "host out-parameter of a planning query",
    ("xp_contrastive_loss_operands", "reads_img"): "host out-parameter of a planning query",
    ("xp_contrastive_loss_operands", "reads_cap"): "host out-parameter of a planning query",
    ("xp_pair_loss_workspace_bytes", "params"): "host struct without pointers",
    ("xp_pair_loss", "params"): "host struct without pointers (travels as kernel arguments)",
    ("xp_encoder_layer_fwd_workspace_bytes", "dims"): "host struct without pointers",
    ("xp_encoder_layer_bwd_workspace_bytes", "dims"): "host struct without pointers",
    ("xp_encoder_layer_pooled_fwd_workspace_bytes", "dims"): "host struct without pointers",
    ("xp_encoder_layer_pooled_bwd_workspace_bytes", "dims"): "host struct without pointers",
}
# host structures whose pointer FIELDS are the operands: (entry, parameter) -> struct; the operand is "parameter.field"
# ("parameter[].field" where the parameter is a host array of them)
HOST_STRUCTS = {
    ("xp_gemm", "desc"): ("XpGemmDesc", "desc."),
    ("xp_reduce_rows_batch", "segs_host"): ("XpReduceSeg", "segs_host[]."),
    ("xp_frames_resize_norm", "videos_host"): ("XpFrameSrc", "videos_host[]."),
    ("xp_frames_transform", "videos_host"): ("XpFrameTransform", "videos_host[]."),
    ("xp_frames_transform_aa", "videos_host"): ("XpFrameTransform", "videos_host[]."),
    ("xp_encoder_layer_fwd", "args"): ("XpLayerFwd", "args."),
    ("xp_encoder_layer_bwd", "args"): ("XpLayerBwd", "args."),
    ("xp_encoder_layer_bwd_listed", "args"): ("XpLayerBwd", "args."),
    ("xp_encoder_layer_bwd_listed", "dx3_support"): ("XpDx3Support", "dx3_support."),
    ("xp_encoder_layer_pooled_fwd", "args"): ("XpLayerPooledFwd", "args."),
    ("xp_encoder_layer_pooled_bwd", "args"): ("XpLayerPooledBwd", "args."),
}
# the optimizer's tensor lists: a DEVICE table of XpAdamTensor (the table itself is an operand; the tensors it names are operands
# "table[].p" ... the host cannot read) and a HOST array of device pointers (operands "grads_host[]")
OPTIM_ENTRIES = ("xp_grad_sqnorm_partials", "xp_adamw_step", "xp_optim_step", "xp_adamw_step_guarded", "xp_optim_step_guarded")
DEVICE_TABLE_FIELDS = {"table": "XpAdamTensor"}
HOST_POINTER_ARRAYS = {"grads_host": "grads_host[]"}
# struct fields that are no device operands
EXEMPT_FIELDS = {
    ("XpGemmDesc", "k_tile_begin_host"): "host copy of k_tile_begin, which the call validates",
    ("XpDx3Support", "k_tile_begin_host"): "host copies of k_tile_begin, which the call validates",
}

# ------------------------------------------------------------------------------------------------------------ the classes
NEED_VEC4 = "need 8/16"
_FRAMES_ANY = "src: bytes, read one at a time or as the aligned dwords around them (tests/test_frame_transform_gpu.py, odd_offset)"
# One row per (entry, operand).  LayerNorm's x, y (forward) and dy, x, dres, dx (backward) move four elements per lane in the
# narrowest kernel (VEC4); xp_gemm's desc.a_frames is the fp32 frame tensor here (decoded uint8 frames, a_frames_u8 = 1: need 8,
# as xp_im2col_u8); xp_grad_sqnorm_partials' partials is one float per workgroup, and optimization/multi_tensor.py hands each
# launch table its slice of the step's array; the optimizer's tensors may be views at any element of a flat buffer
# (distributed.GradBucketReducer's .grad views, a one-element logit_scale).
N16, N8, N4, VEC4, ANY = "need 16", "need 8", "need 4", NEED_VEC4, "any"
ROWS = {
    "xp_gemm": {"desc.A": N16, "desc.B": N16, "desc.C": N16, "desc.bias": N16, "desc.resid": N16, "desc.aux": N16,
        "desc.tab1": N16, "desc.tab2": N16, "desc.colsum_partials": N16, "desc.resid_side": N16, "desc.out_side": N16,
        "desc.a_frames": N16, "desc.m_tiles": N16, "desc.k_tiles": N16, "desc.k_tile_begin": N16},
    "xp_splitk_reduce": {"slabs": N16, "out": N16},
    "xp_colsum": {"X": N16, "out": N16, "workspace": N16},
    "xp_colsum_partials": {"X": N16, "partials": N16},
    "xp_reduce_rows_batch": {"segs_host[].in": ANY, "segs_host[].out": ANY, "workspace": ANY},
    "xp_layernorm_fwd": {"x": VEC4, "gamma": N16, "beta": N16, "y": VEC4, "mean": N16, "rstd": N16},
    "xp_layernorm_fwd_side": {"x": VEC4, "gamma": N16, "beta": N16, "y": VEC4, "mean": N16, "rstd": N16, "x_side": N16,
        "y_side": N16},
    "xp_layernorm_bwd_partials": {"dy": VEC4, "x": VEC4, "gamma": N16, "mean": N16, "rstd": N16, "dres": VEC4, "dx": VEC4,
        "workspace": N16},
    "xp_layernorm_bwd": {"dy": VEC4, "x": VEC4, "gamma": N16, "mean": N16, "rstd": N16, "dres": VEC4, "dx": VEC4,
        "dgamma": N16, "dbeta": N16, "workspace": N16},
    "xp_layernorm_bwd_partials_side": {"dy": VEC4, "x": VEC4, "gamma": N16, "mean": N16, "rstd": N16, "dres": VEC4, "dx": VEC4,
        "x_side": N16, "workspace": N16},
    "xp_layernorm_bwd_side": {"dy": VEC4, "x": VEC4, "gamma": N16, "mean": N16, "rstd": N16, "dres": VEC4, "dx": VEC4,
        "dgamma": N16, "dbeta": N16, "x_side": N16, "workspace": N16},
    "xp_attn_fwd": {"qkv": N16, "out": N16, "stats": N16, "pad_mask": N16, "workspace": N16},
    "xp_attn_bwd": {"qkv": N16, "out": N16, "dout": N16, "stats": N16, "pad_mask": N16, "dqkv": N16, "workspace": N16},
    "xp_attn_bwd2": {"qkv": N16, "out": N16, "dout": N16, "stats": N16, "pad_mask": N16, "dqkv": N16, "workspace": N16,
        "dqkv_colsum_partials": N16},
    "xp_attn_probs": {"qkv": N16, "stats": N16, "pad_mask": N16, "probs": N16, "probs_proxy": N16},
    "xp_attn_pooled_fwd": {"q": N16, "kv": N16, "out": N16, "stats": N16, "workspace": N16},
    "xp_attn_pooled_bwd": {"q": N16, "kv": N16, "out": N16, "dout": N16, "stats": N16, "dq": N16, "dkv": N16, "workspace": N16,
        "dkv_colsum_partials": N16},
    "xp_im2col": {"video": N16, "patches": N16},
    "xp_im2col_u8": {"frames": N8, "patches": N16},
    "xp_frames_resize_norm": {"videos_host[].src": ANY, "out": ANY},
    "xp_frames_transform": {"videos_host[].src": ANY, "out": ANY},
    "xp_frames_transform_aa": {"videos_host[].src": ANY, "out": ANY, "workspace": N4},
    "xp_vip_proxy_rows": {"class_emb": N16, "added_cls": N16, "pos": N16, "x": N16},
    "xp_vip_embed_bwd": {"dx": N16, "d_class": N16, "d_added": N16, "d_pos": N16, "d_time": N16, "workspace": N16},
    "xp_pos_resample_fwd": {"pos": N16, "out": N16},
    "xp_pos_resample_bwd": {"d_out": N16, "d_pos": N16},
    "xp_text_embed_fwd": {"ids": N16, "tok": N16, "pos": N16, "x": N16},
    "xp_text_embed_bwd": {"ids": N16, "dx": N16, "d_tok": N16, "d_pos": N16},
    "xp_text_embed_fwd_pos": {"ids": N16, "pos_ids": N16, "tok": N16, "pos": N16, "x": N16},
    "xp_text_embed_bwd_pos": {"ids": N16, "pos_ids": N16, "dx": N16, "d_tok": N16, "d_pos": N16},
    "xp_argmax_rows": {"ids": N16, "idx": N16},
    "xp_gather_rows": {"x": N16, "idx": N16, "out": N16},
    "xp_scatter_rows": {"dout": N16, "idx": N16, "dx": N16},
    "xp_l2norm_fwd": {"x": N16, "y": N16, "inv_norm": N16},
    "xp_l2norm_bwd": {"dy": N16, "y": N16, "inv_norm": N16, "dx": N16},
    "xp_cast": {"src": N16, "dst": N16},
    "xp_cast_back": {"src": N16, "dst": N16},
    "xp_grad_sqnorm_partials": {"table": N16, "table[].p": ANY, "table[].m": ANY, "table[].v": ANY, "table[].shadow": ANY,
        "chunk_map": N16, "grads_host[]": ANY, "partials": ANY},
    "xp_adamw_step": {"table": N16, "table[].p": ANY, "table[].m": ANY, "table[].v": ANY, "table[].shadow": ANY,
        "chunk_map": N16, "grads_host[]": ANY, "norm_partials": N16, "grad_norm_out": N16},
    "xp_optim_step": {"table": N16, "table[].p": ANY, "table[].m": ANY, "table[].v": ANY, "table[].shadow": ANY,
        "chunk_map": N16, "grads_host[]": ANY, "norm_partials": N16, "grad_norm_out": N16},
    "xp_step_verdict": {"partials": N16, "verdict": N16},
    "xp_adamw_step_guarded": {"table": N16, "table[].p": ANY, "table[].m": ANY, "table[].v": ANY, "table[].shadow": ANY,
        "chunk_map": N16, "grads_host[]": ANY, "norm_partials": N16, "grad_norm_out": N16, "verdict": N16},
    "xp_optim_step_guarded": {"table": N16, "table[].p": ANY, "table[].m": ANY, "table[].v": ANY, "table[].shadow": ANY,
        "chunk_map": N16, "grads_host[]": ANY, "norm_partials": N16, "grad_norm_out": N16, "verdict": N16},
    "xp_contrastive_loss": {"vis": N16, "txt": N16, "img": N16, "cap": N16, "log_scale": N16, "loss": N16, "d_vis": N16,
        "d_txt": N16, "d_img": N16, "d_cap": N16, "d_log_scale": N16, "workspace": N16},
    "xp_pair_loss": {"vis": N16, "txt": N16, "loss": N16, "d_vis": N16, "d_txt": N16, "workspace": N16},
    "xp_sim_matrix": {"a": ANY, "b": ANY, "sim": ANY},
    "xp_dsl_rerank": {"sim": N16},
    "xp_retrieval_ranks": {"sim": N16, "labels": N16, "greater": N16, "equal": N16},
    "xp_retrieval_ranks_streamed": {"q": ANY, "g": ANY, "labels_q": N16, "labels_g": N16, "greater_q": N16, "equal_q": N16,
        "greater_g": N16, "equal_g": N16, "workspace": N16},
    "xp_retrieval_topk": {"q": ANY, "g": ANY, "vals": N16, "idx": N16, "workspace": N16},
    "xp_retrieval_dsl_stats": {"over": ANY, "of": ANY, "mx": N16, "sum": N16, "workspace": N16},
    "xp_retrieval_topk_dsl": {"q": ANY, "g": ANY, "mx": ANY, "sum": ANY, "vals": N16, "idx": N16, "workspace": N16},
    "xp_encoder_layer_fwd": {"args.x": N16, "args.Wqkv": N16, "args.Wo": N16, "args.W1": N16, "args.W2": N16,
        "args.ln1_w": N16, "args.ln1_b": N16, "args.bqkv": N16, "args.bo": N16, "args.ln2_w": N16, "args.ln2_b": N16,
        "args.b1": N16, "args.b2": N16, "args.pad_mask": N16, "args.h1": N16, "args.qkv": N16, "args.attn_o": N16,
        "args.x2": N16, "args.h2": N16, "args.pre": N16, "args.act": N16, "args.x3": N16, "args.mean1": N16, "args.rstd1": N16,
        "args.mean2": N16, "args.rstd2": N16, "args.stats": N16, "args.workspace": N16, "args.side_in": N16,
        "args.side_out": N16, "args.side_x2": N16},
    "xp_encoder_layer_bwd": {"args.x": N16, "args.h1": N16, "args.qkv": N16, "args.attn_o": N16, "args.x2": N16,
        "args.h2": N16, "args.pre": N16, "args.act": N16, "args.Wqkv": N16, "args.Wo": N16, "args.W1": N16, "args.W2": N16,
        "args.ln1_w": N16, "args.ln2_w": N16, "args.mean1": N16, "args.rstd1": N16, "args.mean2": N16, "args.rstd2": N16,
        "args.stats": N16, "args.pad_mask": N16, "args.dx3": N16, "args.dx": N16, "args.dln1_w": N16, "args.dln1_b": N16,
        "args.dwqkv": N16, "args.dbqkv": N16, "args.dwo": N16, "args.dbo": N16, "args.dln2_w": N16, "args.dln2_b": N16,
        "args.dw1": N16, "args.db1": N16, "args.dw2": N16, "args.db2": N16, "args.workspace": N16, "args.side_in": N16,
        "args.side_x2": N16},
    "xp_encoder_layer_bwd_listed": {"args.x": N16, "args.h1": N16, "args.qkv": N16, "args.attn_o": N16, "args.x2": N16,
        "args.h2": N16, "args.pre": N16, "args.act": N16, "args.Wqkv": N16, "args.Wo": N16, "args.W1": N16, "args.W2": N16,
        "args.ln1_w": N16, "args.ln2_w": N16, "args.mean1": N16, "args.rstd1": N16, "args.mean2": N16, "args.rstd2": N16,
        "args.stats": N16, "args.pad_mask": N16, "args.dx3": N16, "args.dx": N16, "args.dln1_w": N16, "args.dln1_b": N16,
        "args.dwqkv": N16, "args.dbqkv": N16, "args.dwo": N16, "args.dbo": N16, "args.dln2_w": N16, "args.dln2_b": N16,
        "args.dw1": N16, "args.db1": N16, "args.dw2": N16, "args.db2": N16, "args.workspace": N16, "args.side_in": N16,
        "args.side_x2": N16, "dx3_support.m_tiles": N16, "dx3_support.k_tiles[0]": N16, "dx3_support.k_tiles[1]": N16,
        "dx3_support.k_tiles[2]": N16, "dx3_support.k_tile_begin[0]": N16, "dx3_support.k_tile_begin[1]": N16,
        "dx3_support.k_tile_begin[2]": N16},
    "xp_encoder_layer_pooled_fwd": {"args.x": N16, "args.Wqkv": N16, "args.Wo": N16, "args.W1": N16, "args.W2": N16,
        "args.ln1_w": N16, "args.ln1_b": N16, "args.bqkv": N16, "args.bo": N16, "args.ln2_w": N16, "args.ln2_b": N16,
        "args.b1": N16, "args.b2": N16, "args.h1": N16, "args.kv": N16, "args.mean1": N16, "args.rstd1": N16, "args.h1p": N16,
        "args.q": N16, "args.attn_o": N16, "args.x2": N16, "args.h2": N16, "args.pre": N16, "args.act": N16, "args.x3": N16,
        "args.mean1p": N16, "args.rstd1p": N16, "args.mean2": N16, "args.rstd2": N16, "args.stats": N16, "args.workspace": N16,
        "args.side_in": N16, "args.side_out": N16, "args.side_x2": N16},
    "xp_encoder_layer_pooled_bwd": {"args.x": N16, "args.h1": N16, "args.kv": N16, "args.h1p": N16, "args.q": N16,
        "args.attn_o": N16, "args.x2": N16, "args.h2": N16, "args.pre": N16, "args.act": N16, "args.Wqkv": N16, "args.Wo": N16,
        "args.W1": N16, "args.W2": N16, "args.ln1_w": N16, "args.ln2_w": N16, "args.mean1": N16, "args.rstd1": N16,
        "args.mean1p": N16, "args.rstd1p": N16, "args.mean2": N16, "args.rstd2": N16, "args.stats": N16, "args.dx3": N16,
        "args.dx": N16, "args.dln1_w": N16, "args.dln1_b": N16, "args.dwqkv": N16, "args.dbqkv": N16, "args.dwo": N16,
        "args.dbo": N16, "args.dln2_w": N16, "args.dln2_b": N16, "args.dw1": N16, "args.db1": N16, "args.dw2": N16,
        "args.db2": N16, "args.workspace": N16, "args.side_in": N16, "args.side_x2": N16},
    "xp_debug_set_gemm_trace": {"device_buffer": N16},
    "xp_debug_set_attn_trace": {"device_buffer": N16},
    "xp_probe_mfma_bf16": {"a": N16, "b": N16, "c": N16},
    "xp_probe_mfma_f32": {"a": N16, "b": N16, "c": N16},
    "xp_probe_pk_f32": {"err": N16},
    "xp_probe_stream_copy": {"dst": N16, "src": N16},
    "xp_probe_stream_copy_fat": {"dst": N16, "src": N16},
    "xp_probe_tr16": {"in": N16, "lane_byte_off": N16, "out": N16},
}
# what the GPU test holds a misaligned run of an ``any`` operand to: "same": the aligned run's bits (the same kernel, or kernels
# whose bits the entry's contract makes equal); otherwise the existing reference and the test whose tolerance is taken
ANY_HELD_TO = {
    "xp_sim_matrix": "same (one kernel, sgemm_strided_kernel)",
    "xp_reduce_rows_batch": "same: reduce_batch_kernel<1, .> and <4, .> run one tree per column (tests/test_reduce_gpu.py holds them bit-equal)",
    "xp_retrieval_ranks_streamed": "same: a score's bits depend on its two rows and d alone (include/xpretrain_hip.h; tests/test_retrieval_stream_gpu.py)",
    "xp_retrieval_topk": "same, as above",
    "xp_retrieval_topk_dsl": "same, as above; mx and sum are read one float per lane, and a gallery fed shard by shard gets its slice of "
                             "them (tests/test_retrieval_dsl_gpu.py::test_shards_equal_one_shot_given_the_statistics)",
    "xp_retrieval_dsl_stats": "same, as above",
    "xp_frames_resize_norm": "same (one kernel; out is stored one float per pixel); " + _FRAMES_ANY,
    "xp_frames_transform": "same (one kernel per filter); " + _FRAMES_ANY,
    "xp_frames_transform_aa": "same (one kernel pair); " + _FRAMES_ANY,
    **{e: "same without clipping (the update is element by element; tests/test_optim_family_gpu.py holds the misaligned tensor to live "
          "torch); the norm partials to the fp64 sum at that test's 1e-5" for e in OPTIM_ENTRIES},
}

# ------------------------------------------------------------------------------------------------------------ the smallest calls
WS = 8 << 20                       # workspace_bytes of every call below (the GPU test's workspace buffers are this large)
_DIMS = dict(rows=32, D=64, Dff=128, B=2, S=16, heads=1, M=1, N=3, L=5, attn_mode=0, dtype=BF16, q_scale=0.125, ln_eps=1e-5, act=0)
_ATTN = dict(mode=0, B=2, H=1, S=16, M=1, N=3, L=5, dtype=BF16, workspace_bytes=WS)
_LN = dict(ldx=128, ldy=128, rows=5, cols=128, eps=1e-5)
_LNB = dict(lddy=128, ldx=128, lddres=128, lddx=128, rows=5, cols=128, workspace_bytes=WS)
_SIDE = dict(side_S=5, side_M=1, side_stride=1)
_OPT = dict(n_chunks=1, n_tensors=1, n_groups=1, n_norm_partials=1, max_norm=1.0)
_FRAME_SRC = dict(src_bytes=8 * 8 * 3, stride_t=8 * 8 * 3, stride_y=8 * 3, stride_x=3, stride_c=1, T=1, H=8, W=8, box_y=0, box_x=0,
                  box_h=8, box_w=8, rh=4, rw=4, top=0, left=0, flip=0)
_FRAMES = dict(n_videos=1, oh=4, ow=4)
# entry -> dict(args by header name; "dtypes": the storage types the call is made with (default: the one in args);
#               "null": operands left NULL in the base call; "esz": element sizes that the C type does not say)
CALLS = {
    "xp_gemm": dict(desc=dict(M=128, N=128, K=128, lda=128, ldb=128, ldc=128, ldr=128, ldaux=128, in_dtype=BF16, out_dtype=BF16,
                              epilogue=3, split_k=1, scale=1.0),
                    null=("desc.resid", "desc.tab1", "desc.tab2", "desc.colsum_partials", "desc.resid_side", "desc.out_side",
                          "desc.a_frames", "desc.m_tiles", "desc.k_tiles", "desc.k_tile_begin"),
                    esz={"desc.a_frames": 4}),
    "xp_splitk_reduce": dict(n=128, splits=2, accumulate=0),
    "xp_colsum": dict(rows=8, cols=128, ldx=128, dtype=BF16, accumulate=0, workspace_bytes=WS),
    "xp_colsum_partials": dict(rows=8, cols=128, ldx=128, dtype=BF16, partials_bytes=WS),
    "xp_reduce_rows_batch": dict(n=1, workspace_bytes=WS, segs_host=dict(stride=8, nrows=3, width=8)),
    "xp_layernorm_fwd": dict(_LN, dtypes=(BF16, F32)),
    "xp_layernorm_fwd_side": dict(_LN, **_SIDE, dtypes=(BF16, F32)),
    "xp_layernorm_bwd_partials": dict(_LNB, with_dx_colsum=0, dtypes=(BF16, F32)),
    "xp_layernorm_bwd": dict(_LNB, accumulate=0, dtypes=(BF16, F32)),
    "xp_layernorm_bwd_partials_side": dict(_LNB, with_dx_colsum=0, **_SIDE, dtypes=(BF16, F32)),
    "xp_layernorm_bwd_side": dict(_LNB, accumulate=0, **_SIDE, dtypes=(BF16, F32)),
    "xp_attn_fwd": dict(_ATTN, ldqkv=192, ldo=64, null=("pad_mask",)),
    "xp_attn_bwd": dict(_ATTN, ldqkv=192, ldo=64, q_scale=0.125, null=("pad_mask",)),
    "xp_attn_bwd2": dict(_ATTN, ldqkv=192, ldo=64, q_scale=0.125, null=("pad_mask", "dqkv_colsum_partials")),
    "xp_attn_probs": dict({k: v for k, v in _ATTN.items() if k != "workspace_bytes"}, ldqkv=192, null=("pad_mask",)),
    "xp_attn_pooled_fwd": dict(ldkv=128, B=2, H=1, S=16, dtype=BF16, workspace_bytes=WS),
    "xp_attn_pooled_bwd": dict(ldkv=128, lddq=64, lddkv=128, q_scale=0.125, B=2, H=1, S=16, dtype=BF16, workspace_bytes=WS,
                               null=("dkv_colsum_partials",)),
    "xp_im2col": dict(BT=1, H=16, W=16, P=8, dtype=BF16),
    "xp_im2col_u8": dict(BT=1, H=16, W=16, P=8, dtype=BF16),
    "xp_frames_resize_norm": dict(_FRAMES, videos_host=_FRAME_SRC),
    "xp_frames_transform": dict(_FRAMES, videos_host=dict(src=_FRAME_SRC, filter=0)),
    "xp_frames_transform_aa": dict(_FRAMES, videos_host=dict(src=_FRAME_SRC, filter=0), workspace_bytes=WS),
    "xp_vip_proxy_rows": dict(B=2, S=17, M=2, D=128, dtype=BF16),
    "xp_vip_embed_bwd": dict(B=2, M=2, T=3, L=5, D=128, dtype=BF16, accumulate=0, workspace_bytes=WS),
    "xp_pos_resample_fwd": dict(g0=2, gh=3, gw=3, D=4),
    "xp_pos_resample_bwd": dict(g0=2, gh=3, gw=3, D=4),
    "xp_text_embed_fwd": dict(B=2, Lt=4, D=128, vocab=10, dtype=BF16),
    "xp_text_embed_bwd": dict(B=2, Lt=4, D=128, vocab=10, dtype=BF16, accumulate=1),
    "xp_text_embed_fwd_pos": dict(pos_B=1, B=2, Lt=4, D=128, vocab=10, n_pos=8, dtype=BF16),
    "xp_text_embed_bwd_pos": dict(pos_B=1, B=2, Lt=4, D=128, vocab=10, n_pos=8, dtype=BF16, accumulate=1),
    "xp_argmax_rows": dict(B=2, Lt=4),
    "xp_gather_rows": dict(B=2, S=4, D=128, dtype=BF16),
    "xp_scatter_rows": dict(B=2, S=4, D=128, dtype=BF16),
    "xp_l2norm_fwd": dict(rows=2, cols=128, dtype=BF16),
    "xp_l2norm_bwd": dict(rows=2, cols=128, dtype=BF16),
    "xp_cast": dict(n=128, dtype=BF16),
    "xp_cast_back": dict(n=128, dtype=BF16, accumulate=0),
    "xp_grad_sqnorm_partials": dict(n_chunks=1, n_tensors=1),
    "xp_adamw_step": dict(_OPT),
    "xp_optim_step": dict(_OPT, kind=0),
    "xp_step_verdict": dict(n_partials=1),
    "xp_adamw_step_guarded": dict(_OPT),
    "xp_optim_step_guarded": dict(_OPT, kind=0),
    "xp_contrastive_loss": dict(kind=0, n=4, m=4, d=8, workspace_bytes=WS, null=("img", "cap", "d_img", "d_cap")),
    "xp_pair_loss": dict(kind=0, params=dict(temp=0.1, margin=0.2, hard_negative_num=1, bag=1), n=4, d=8, workspace_bytes=WS),
    "xp_sim_matrix": dict(na=4, nb=4, d=8),
    "xp_dsl_rerank": dict(n=4, m=4, theta=1.0, multiply=1),
    "xp_retrieval_ranks": dict(n=4, m=4, transpose=0, null=("labels",)),
    "xp_retrieval_ranks_streamed": dict(nq=4, ng=4, d=8, dsl=0, theta=1.0, workspace_bytes=WS, null=("labels_q", "labels_g")),
    "xp_retrieval_topk": dict(nq=4, ng=4, d=8, k=2, index_base=0, accumulate=0, workspace_bytes=WS),
    "xp_retrieval_dsl_stats": dict(n_over=4, n_of=4, d=8, theta=1.0, accumulate=0, workspace_bytes=WS),
    "xp_retrieval_topk_dsl": dict(nq=4, ng=4, d=8, k=2, index_base=0, accumulate=0, theta=1.0, stats_of=1, workspace_bytes=WS),
    "xp_encoder_layer_fwd": dict(args=dict(dims=_DIMS, workspace_bytes=WS), null=("args.pad_mask", "args.side_in", "args.side_out", "args.side_x2")),
    "xp_encoder_layer_bwd": dict(args=dict(dims=_DIMS, workspace_bytes=WS), null=("args.pad_mask", "args.side_in", "args.side_x2")),
    "xp_encoder_layer_bwd_listed": dict(args=dict(dims=_DIMS, workspace_bytes=WS), dx3_support=dict(n_m_tiles=1, split=(1, 1, 1), k_tile_begin_host=True),
                                        null=("args.pad_mask", "args.side_in", "args.side_x2"), base_unchecked=True),
    "xp_encoder_layer_pooled_fwd": dict(args=dict(dims=_DIMS, workspace_bytes=WS), null=("args.side_in", "args.side_out", "args.side_x2")),
    "xp_encoder_layer_pooled_bwd": dict(args=dict(dims=_DIMS, workspace_bytes=WS), null=("args.side_in", "args.side_x2")),
    "xp_debug_set_gemm_trace": dict(esz={"device_buffer": 8}, setter=True),
    "xp_debug_set_attn_trace": dict(esz={"device_buffer": 8}, setter=True),
    "xp_probe_mfma_bf16": dict(esz={"a": 2, "b": 2}),
    "xp_probe_mfma_f32": dict(),
    "xp_probe_pk_f32": dict(iters=1, blocks=1, seed=0, esz={"err": 4}),
    "xp_probe_stream_copy": dict(nbytes=16, blocks=1, iters=1, esz={"dst": 1, "src": 1}),
    "xp_probe_stream_copy_fat": dict(nbytes=16, blocks=1, iters=1, esz={"dst": 1, "src": 1}),
    "xp_probe_tr16": dict(esz={"in": 2, "out": 2}),
}
# "setter": the entry only stores the pointer (returns 0); "base_unchecked": the aligned call is not made on its own -- the listed
# backward needs the 256-wide-family plans of a full-size layer and tile lists cut by them (tests/test_tile_lists_gpu.py runs it)
_META = ("dtypes", "null", "esz", "setter", "base_unchecked")
# The one operand whose N depends on an argument other than the storage type: xp_gemm's desc.a_frames is need 16 for fp32 frames
# (the ROWS entry, CALLS["xp_gemm"]) and need 8 for decoded uint8 frames -- this variant of the call: 2 frames of 16 x 16 at patch 8
# (M = 8 patches, K = 3 * 8 * 8), A itself absent, gathered by the operand loader.
GEMM_U8_FRAMES = dict(desc=dict(M=8, N=128, K=192, lda=192, ldb=192, ldc=128, ldr=128, ldaux=128, in_dtype=BF16, out_dtype=BF16, epilogue=0,
                                split_k=1, scale=1.0, a_frames_u8=1, fr_H=16, fr_W=16, fr_P=8, fr_mean=(0.5, 0.5, 0.5), fr_std=(0.25, 0.25, 0.25)),
                      null=("desc.A", "desc.bias", "desc.resid", "desc.aux", "desc.tab1", "desc.tab2", "desc.colsum_partials", "desc.resid_side",
                            "desc.out_side", "desc.m_tiles", "desc.k_tiles", "desc.k_tile_begin"))
GEMM_U8_FRAMES_NEED = ("desc.a_frames", 8, (1, 2, 4))           # operand, N, the refused offsets (uint8: one element and the powers below N)
_CSIZE = {"float": 4, "int32_t": 4, "int64_t": 8, "uint8_t": 1, "XpStepVerdict": 8, "XpAdamTensor": 8}


# ------------------------------------------------------------------------------------------------------------ rows
def operands(entry, protos=None, structs=None):
    """[(operand, base C type)] of an entry: its pointer parameters and the pointer fields of its host structs, without the
    exempt ones; raises KeyError for a pointer that is neither in a table here nor exempt"""
    protos, structs = protos or prototypes(), structs or struct_fields()
    out = []
    for ctype, name, is_ptr in protos[entry]:
        if not is_ptr or name in EXEMPT_NAMES or (entry, name) in EXEMPT:
            continue
        base = ctype.replace("const", "").replace("*", "").strip()
        if (entry, name) in HOST_STRUCTS:
            sname, prefix = HOST_STRUCTS[(entry, name)]
            out += _struct_operands(sname, prefix, structs)
        elif name in HOST_POINTER_ARRAYS and entry in OPTIM_ENTRIES:
            out.append((HOST_POINTER_ARRAYS[name], "float"))
        else:
            if base in structs and base not in ("XpStepVerdict", "XpAdamTensor"):
                raise KeyError(f"{entry}({name}): a {base}* that is neither in HOST_STRUCTS nor in EXEMPT")
            out.append((name, base))
            if name in DEVICE_TABLE_FIELDS and entry in OPTIM_ENTRIES:
                out += _struct_operands(DEVICE_TABLE_FIELDS[name], name + "[].", structs, base="float")
    return out


def _struct_operands(sname, prefix, structs, base=None):
    out = []
    for fbase, fname, is_ptr, n in structs[sname]:
        if fbase in structs and not is_ptr:                      # a nested struct (XpFrameTransform.src, XpLayer*.dims)
            out += _struct_operands(fbase, prefix + fname + ".", structs)
        elif is_ptr and (sname, fname) not in EXEMPT_FIELDS:
            names = [f"{prefix}{fname}[{i}]" for i in range(n)] if n else [prefix + fname]
            out += [(x, base or fbase) for x in names]
    # the frame descriptors nest XpFrameSrc: its pointer is "videos_host[].src" whatever the nesting
    return [(re.sub(r"\.src\.src$", ".src", o), b) for o, b in out]


def class_of(entry, operand):
    return ROWS[entry][operand]


def need_bytes(cls, dtype):
    """N of a ``need`` class for a call made with storage type ``dtype``; None for ``any``"""
    if cls == "any":
        return None
    if cls == NEED_VEC4:
        return 8 if dtype == BF16 else 16
    return int(cls.split()[1])


def call_dtypes(entry):
    c = CALLS[entry]
    if "dtypes" in c:
        return c["dtypes"]
    for holder in (c, c.get("desc", {}), c.get("args", {}).get("dims", {})):
        for k in ("dtype", "in_dtype"):
            if k in holder:
                return (holder[k],)
    return (F32,)


def element_size(entry, operand, ctype, dtype):
    esz = CALLS[entry].get("esz", {})
    if operand in esz:
        return esz[operand]
    if operand.split(".")[-1] == "workspace":
        return 1
    if ctype == "void":
        return 2 if dtype == BF16 else 4
    return _CSIZE[ctype]


def refused_offsets(n, esz):
    """the byte offsets a ``need n`` operand is refused at: one element, and 8 bytes where n is 16"""
    return sorted({o for o in (esz, 8) if o % n})


def need_rows():
    """[(entry, operand, dtype, N, [offsets])] of every refusal the tests make"""
    protos, structs, out = prototypes(), struct_fields(), []
    for entry in CALLS:
        for operand, ctype in operands(entry, protos, structs):
            for dtype in call_dtypes(entry):
                n = need_bytes(class_of(entry, operand), dtype)
                if n is not None:
                    out.append((entry, operand, dtype, n, refused_offsets(n, element_size(entry, operand, ctype, dtype))))
    return out


# ------------------------------------------------------------------------------------------------------------ a row as a call
def build_call(entry, dtype, address, extra=(), spec=None):
    """(arguments in header order, keep-alive list) of CALLS[entry] (or of ``spec``, a variant of it) with storage type ``dtype``;
    ``address(operand)`` gives the device address of an operand.  Operands in the call's ``null`` stay NULL unless named in ``extra``."""
    from xpretrain_amd import _lib as L
    spec, keep = spec or CALLS[entry], []
    null = set(spec.get("null", ())) - set(extra)
    protos, structs = prototypes(), struct_fields()
    argtypes = L.SIGNATURES[entry][1]

    def addr(op):
        return 0 if op in null else address(op)

    def fill(sname, prefix, values):
        s = getattr(L, sname)()
        values = dict(values)
        for fbase, fname, is_ptr, n in structs[sname]:
            py = fname + "_" * (fname in ("in",))
            if fbase in structs and not is_ptr:
                sub = fill(fbase, prefix + fname + ".", values.pop(fname, {}))
                setattr(s, py, sub)
            elif is_ptr and (sname, fname) in EXEMPT_FIELDS:
                if values.pop(fname, None):                              # host memory: a real array
                    host = (C.c_int32 * 8)(0, 2, 4, 6, 8, 10, 12, 14)
                    keep.append(host)
                    for i in range(n):
                        getattr(s, py)[i] = C.addressof(host)
            elif is_ptr:
                op = re.sub(r"\.src\.src$", ".src", prefix + fname)
                if n:
                    for i in range(n):
                        getattr(s, py)[i] = addr(f"{op}[{i}]")
                else:
                    setattr(s, py, addr(op))
            elif fname in values:
                v = values.pop(fname)
                if n:
                    for i, x in enumerate(v):
                        getattr(s, py)[i] = x
                else:
                    setattr(s, py, v)
        for k in ("dtype", "in_dtype", "out_dtype"):
            if any(f[1] == k for f in structs[sname]) and (k != "out_dtype" or getattr(s, k) != F32):
                setattr(s, k, dtype)
        assert not values, (entry, sname, values)
        return s

    args = []
    for (ctype, name, is_ptr), at in zip(protos[entry], argtypes):
        base = ctype.replace("const", "").replace("*", "").strip()
        if not is_ptr:
            args.append(dtype if name == "dtype" else spec[name])
        elif name == "stream":
            args.append(None)
        elif name in ("mean3_host", "std3_host"):
            keep.append((C.c_float * 3)(0.5, 0.5, 0.5))
            args.append(C.cast(keep[-1], C.c_void_p))
        elif name == "group_of_host":
            keep.append((C.c_uint8 * 1)(0))
            args.append(C.cast(keep[-1], C.c_void_p))
        elif name == "groups_host":
            g = getattr(L, base)()
            g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.step_size = 1e-3, 0.9, 0.999, 1e-8, 0.0, 1e-3
            keep.append(g)
            args.append(C.byref(g))
        elif name == "grads_host":
            keep.append((C.c_void_p * 1)(address("grads_host[]")))
            args.append(C.cast(keep[-1], C.c_void_p))
        elif (entry, name) in HOST_STRUCTS:
            s = fill(HOST_STRUCTS[(entry, name)][0], HOST_STRUCTS[(entry, name)][1], spec.get(name, {}))
            keep.append(s)
            args.append(C.byref(s))
        elif (entry, name) in EXEMPT:                                  # a host struct without pointers
            s = getattr(L, base)()
            for k, v in spec[name].items():
                setattr(s, k, v)
            keep.append(s)
            args.append(C.byref(s))
        else:
            a = addr(name)
            args.append(C.cast(C.c_void_p(a), at) if at is not C.c_void_p else (C.c_void_p(a) if a else None))
    return args, keep
