"""The CSV cutter's field converters (``ops/csrc/hip/csv_parse_dev.h``) on the device, field by
field and bit for bit against Python (``_cut_cases.fast_model``: the accepted set, ``int(digits)``,
the fractional digit count and the bits of the correctly rounded ``float(text)``).

The host check (tests/native/swar16_check.cpp) compiles the header with its portable fallbacks;
here it is compiled through hipRTC behind exactly the macro preludes production uses
(``scancut.PRELUDE``: udot4, umul24, alignbit, perm and the asm barrier; ``scanfuse.prelude``: udot4,
umul24 and the LDS power-of-ten table), with the cutter's LDS table of 10^k and RN(10^-k).  One
field per thread out of a staged LDS buffer, two builds, one launch each.

Fields: every length 1..16, every dot position, the three sign variants, leading zeros, 9-digit
mantissas, for each fr = 1..9 mantissas whose one-multiply quotient is not the rounded quotient
(64 per fr; a CPU loop finds 2 677 to 10 604 such among 20 000 random mantissas, depending on fr),
and every byte value 0..255 substituted at every position of valid fields of each length; each at
all four ``end mod 4``, ``end mod 16`` from 4 to 11, with digits, a dot, signs, 0xFF, a quote or a
separator in the bytes around it.  587 132 placed fields in all: the 16-byte converters see all of
them, the 8-byte ones the 144 452 to 166 956 that fit their frame."""
import numpy as np
import pytest
import torch

import _cut_cases as cc

pytestmark = pytest.mark.gpu

ENTRY = "dq_conv_probe"
BLOCK_BYTES = 256 * cc.SLOT
C_INT, C_DOUBLE = 1, 4
NOT_RUN = 0x80000000

_STAGE = f"""
using namespace dq4ml_csv;
typedef unsigned int csv_u32x4 __attribute__((ext_vector_type(4)));
struct DqPtrs {{ void* v[3]; }};
__device__ __forceinline__ void put(unsigned int* o, bool ok, bool neg, bool dot, int fr, unsigned int m, double dv) {{
  o[0] = (ok ? 1u : 0u) | (neg ? 2u : 0u) | (dot ? 4u : 0u) | (((unsigned int)fr & 0xFFu) << 8);
  o[1] = m;
  o[2] = (unsigned int)__double2loint(dv);
  o[3] = (unsigned int)__double2hiint(dv);
}}
extern "C" __global__ __launch_bounds__(256) void {ENTRY}(const DqPtrs P, long long n) {{
  const unsigned char* __restrict__ src = (const unsigned char*)P.v[0];
  const int* __restrict__ fld = (const int*)P.v[1];
  unsigned int* __restrict__ out = (unsigned int*)P.v[2];
  __shared__ __attribute__((aligned(16))) unsigned char stage_raw[16 + {BLOCK_BYTES} + 32];
  unsigned char* const stage = stage_raw + 16;  // 16 readable bytes below stage[0], as the cutter
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * {BLOCK_BYTES};
  if (tid < 4) reinterpret_cast<unsigned int*>(stage_raw)[tid] = 0u;
  if (tid < 8) reinterpret_cast<unsigned int*>(stage + {BLOCK_BYTES})[tid] = 0u;
#pragma unroll
  for (int j = 0; j < {cc.SLOT // 16}; ++j)
    *reinterpret_cast<csv_u32x4*>(stage + {cc.SLOT} * tid + 16 * j) =
        *reinterpret_cast<const csv_u32x4*>(src + base + {cc.SLOT} * tid + 16 * j);
"""


def _cut_harness():
    from net.jgp.labs.sparkdq4ml_amd.ops import scancut, scanfuse

    body = f"""{scancut.P10_TABLE}  __syncthreads();
  const long long f = (long long)blockIdx.x * 256 + tid;
  if (f >= n) return;
  const int end = fld[2 * f] - (int)base, len = fld[2 * f + 1], start = end - len;
  unsigned int* o = out + f * 24;
  {{  // the 8-byte-frame converters exactly as the cutter's conversion loop calls them
    const int q_fsh = (end - 8) & 3;
    const unsigned* q_wp = reinterpret_cast<const unsigned*>(stage + (end - 8 - q_fsh));
    const unsigned fw0 = q_wp[0], fw1 = q_wp[1], fw2 = q_wp[2];
    const int c0 = stage[start];
    const bool neg0 = c0 == '-';
    const int fl = len - ((c0 == '-' || c0 == '+') ? 1 : 0);
    o[0] = o[4] = {NOT_RUN}u;
    if (fl <= 8) {{
      {{
        unsigned m = 0u;
        int fr = 0;
        bool dot = false;
        const bool ok = csv_num_r8q_w(fw0, fw1, fw2, q_fsh, fl, m, fr, dot);
        const double v = {scancut.DIV_EXPR};
        put(o, ok, neg0, dot, fr, m, neg0 ? -v : v);
      }}
      {{
        unsigned m = 0u;
        int fr = 0;
        bool dot = false;
        const bool ok = csv_num_r8s_w(fw0, fw1, fw2, q_fsh, fl, m, fr, dot);
        const double v = {scancut.DIV_EXPR};
        put(o + 4, ok, neg0, dot, fr, m, neg0 ? -v : v);
      }}
    }}
  }}
  {{
    unsigned m = 0u;
    int fr = 0;
    bool neg = false, dot = false;
    const bool ok = csv_num_r<4>(stage, end, len, m, fr, neg, dot);
    const double v = {scancut.DIV_EXPR};
    put(o + 8, ok, neg, dot, fr, m, neg ? -v : v);
  }}
  o[12] = {NOT_RUN}u;
  if (len <= 8) {{
    unsigned m = 0u;
    int fr = 0;
    bool neg = false, dot = false;
    const bool ok = csv_num_r<2>(stage, end, len, m, fr, neg, dot);
    const double v = {scancut.DIV_EXPR};
    put(o + 12, ok, neg, dot, fr, m, neg ? -v : v);
  }}
  {{
    double dv;
    long long lv;
    int ty;
    const bool ok = csv_field_r16(stage, end, len, dv, lv, ty);
    put(o + 16, ok, false, false, ty, (unsigned int)lv, dv);
  }}
  o[20] = {NOT_RUN}u;
  if (len <= 8) {{
    double dv;
    long long lv;
    int ty;
    const bool ok = csv_field_r8(stage, end, len, dv, lv, ty);
    put(o + 20, ok, false, false, ty, (unsigned int)lv, dv);
  }}
}}
"""
    return scancut.PRELUDE + scanfuse.header_text() + _STAGE + body


def _swar_harness():
    from net.jgp.labs.sparkdq4ml_amd.ops import scanfuse

    body = f"""{scanfuse.P10_INIT}  __syncthreads();
  const long long f = (long long)blockIdx.x * 256 + tid;
  if (f >= n) return;
  const int end = fld[2 * f] - (int)base, len = fld[2 * f + 1], start = end - len;
  unsigned int* o = out + f * 24;
  unsigned long long lo, hi;
  csv_line16(stage, start, lo, hi);  // the field as the first bytes of a short line
  o[0] = {NOT_RUN}u;
  if (len <= 8) {{
    double dv;
    long long lv;
    int ty;
    const bool ok = csv_swar_field(csv_bytes8(lo, hi, 0), len, dv, lv, ty);
    put(o, ok, false, false, ty, (unsigned int)lv, dv);
  }}
  {{
    double dv;
    long long lv;
    int ty;
    const bool ok = csv_swar_field16(lo, hi, len, dv, lv, ty);
    put(o + 4, ok, false, false, ty, (unsigned int)lv, dv);
  }}
}}
"""
    return scanfuse.prelude(True) + scanfuse.header_text() + _STAGE + body


def _run(src, buf, end, ln):
    from net.jgp.labs.sparkdq4ml_amd.ops import dqvm, native

    h = native.hip()
    n = int(end.size)
    nblk = (n + 255) // 256
    padded = np.zeros(nblk * BLOCK_BYTES, np.uint8)
    padded[:buf.size] = buf
    dbuf = torch.from_numpy(padded).cuda()
    dfld = torch.from_numpy(np.stack([end, ln], axis=1).astype(np.int32).copy()).cuda()
    dout = torch.zeros(n * 24, dtype=torch.int32, device="cuda")
    handle = int(h.rtc_compile(src, ENTRY)[0])
    dqvm.launch(h, handle, nblk, [dbuf.data_ptr(), dfld.data_ptr(), dout.data_ptr()], n,
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dout.cpu().numpy().view(np.uint32).reshape(n, 6, 4)


@pytest.fixture(scope="module")
def probe():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    buf, end, ln, uid, texts = cc.convert_layout()
    exp = cc.convert_expected(texts)
    first = np.asarray([t[:1] in (b"+", b"-") for t in texts])[uid]
    res = {"cut": _run(_cut_harness(), buf, end, ln), "swar": _run(_swar_harness(), buf, end, ln)}
    return {"res": res, "len": ln, "fl": ln - first, "uid": uid, "texts": texts, "exp": exp, "end": end, "buf": buf}


def _show(p, idx):
    out = []
    for i in idx[:8]:
        e, n = int(p["end"][i]), int(p["len"][i])
        out.append((p["texts"][p["uid"][i]], e % 16, bytes(p["buf"][e - n - 1:e + 1].tobytes())))
    return out


# (converter, build, record, applies to): the last as the cutter and the scan use each converter
NUM = [("csv_num_r8q_w", "cut", 0, "fl8"), ("csv_num_r8s_w", "cut", 1, "fl8"), ("csv_num_r<4>", "cut", 2, "all"),
       ("csv_num_r<2>", "cut", 3, "len8")]
FIELD = [("csv_field_r16", "cut", 4, "all"), ("csv_field_r8", "cut", 5, "len8"), ("csv_swar_field", "swar", 0, "len8"),
         ("csv_swar_field16", "swar", 1, "all")]


def _domain(p, dom):
    return {"all": np.ones(p["len"].size, bool), "len8": p["len"] <= 8, "fl8": p["fl"] <= 8}[dom]


def _common(p, name, build, rec, dom):
    r = p["res"][build][:, rec, :]
    inside = _domain(p, dom)
    ran = r[:, 0] != NOT_RUN
    assert np.array_equal(ran, inside), name
    ok_e, m_e, fr_e, neg_e, dot_e, bits_e = (a[p["uid"]] for a in p["exp"])
    ok = (r[:, 0] & 1) != 0
    wrong = np.nonzero(inside & (ok != ok_e))[0]
    assert wrong.size == 0, (name, "accepted set", wrong.size, _show(p, wrong))
    sel = inside & ok_e
    bits = r[:, 2].astype(np.uint64) | (r[:, 3].astype(np.uint64) << np.uint64(32))
    wrong = np.nonzero(sel & (bits != bits_e))[0]
    assert wrong.size == 0, (name, "value bits", wrong.size, _show(p, wrong))
    print(f"{name}: {int(inside.sum())} fields checked, {int(sel.sum())} accepted")
    return r, sel, (m_e, fr_e, neg_e, dot_e)


@pytest.mark.parametrize("name,build,rec,dom", NUM, ids=[c[0] for c in NUM])
def test_number_converter_matches_python(probe, name, build, rec, dom):
    p = probe
    r, sel, (m_e, fr_e, neg_e, dot_e) = _common(p, name, build, rec, dom)
    for what, got, want in (("m", r[:, 1].astype(np.int64), m_e), ("fr", ((r[:, 0] >> 8) & 0xFF).astype(np.int32), fr_e),
                            ("neg", (r[:, 0] & 2) != 0, neg_e), ("dot", (r[:, 0] & 4) != 0, dot_e)):
        wrong = np.nonzero(sel & (got != want))[0]
        assert wrong.size == 0, (name, what, wrong.size, _show(p, wrong))


@pytest.mark.parametrize("name,build,rec,dom", FIELD, ids=[c[0] for c in FIELD])
def test_field_converter_matches_python(probe, name, build, rec, dom):
    p = probe
    r, sel, (m_e, fr_e, neg_e, dot_e) = _common(p, name, build, rec, dom)
    lv = r[:, 1].view(np.int32).astype(np.int64)
    lv_e = np.where(dot_e, 0, np.where(neg_e, -m_e, m_e))
    ty_e = np.where(dot_e, C_DOUBLE, C_INT)
    for what, got, want in (("lv", lv, lv_e), ("class", ((r[:, 0] >> 8) & 0xFF).astype(np.int64), ty_e)):
        wrong = np.nonzero(sel & (got != want))[0]
        assert wrong.size == 0, (name, what, wrong.size, _show(p, wrong))


def test_case_set_is_what_the_docstring_says(probe):
    """Counts of the case set: placements, lengths, and the quotient-miss mantissas per fr."""
    p = probe
    miss, counts, tried = cc.quotient_miss_mantissas()
    print("quotient misses among", tried, "random mantissas per fr:", counts)
    assert all(len(miss[fr]) == 64 for fr in range(1, 10))
    assert set(np.unique(p["end"] % 4)) == {0, 1, 2, 3} and np.unique(p["end"] % 16).size >= 8
    ok_e = p["exp"][0][p["uid"]]
    assert set(np.unique(p["len"])) == set(range(1, 17))
    assert set(np.unique(p["len"][ok_e])) == set(range(1, 12))  # sign + 9 digits + dot at the most
    assert set(np.unique(p["exp"][2][p["exp"][0]])) == set(range(10))  # every fr
    assert 2e5 <= p["len"].size <= 8e5
