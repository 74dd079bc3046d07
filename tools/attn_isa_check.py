"""Instruction census of attn_f16x3_kernel and a check of its hand-waited LDS reads, from the compiler's assembly (no GPU).

  hipcc <flags of build.py> -S --cuda-device-only csrc/w2v2_encoder.hip -o enc.s
  python tools/attn_isa_check.py enc.s

Census per instance: vector-ALU instructions outside the matrix pipe, v_exp_f32, packed-fp32 ones, MFMAs, LDS reads and
writes, global stores by width, and the vector instructions per score (128 scores per lane).

Check: the kernel's transposed reads (ds_read_b64_tr_b16) are inline asm, so the compiler does not know that their
destination registers are filled later; the kernel waits for them with counted `s_waitcnt lgkmcnt(N)`.  The scan walks the
instructions in program order, keeps the LDS operations in flight (they return in order; scalar loads in flight make any
count but 0 worthless) and reports every instruction that names a destination register of a transposed read still in flight:
a copy or a use placed in front of the wait would take stale data."""
import re
import sys


def regs(tok):
    """v12 or v[12:15] -> the set of VGPR numbers"""
    out = set()
    for m in re.finditer(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", tok):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_ZN4rsaf4w2v217attn_f16x3_kernel\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name:
            if line.startswith(".Lfunc_end"):
                yield name, body
                name = None
                continue
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                body.append(s)


def check(body):
    census = dict(valu=0, exp=0, pk=0, mfma=0, tr=0, ds_read=0, ds_write=0, ds_other=0)
    stores = {}
    flight, smem, bad = [], 0, []          # flight: [(is_tr, dst regs)] oldest first
    for ins in body:
        op, _, rest = ins.partition(" ")
        live = set().union(*[d for t, d in flight if t]) if flight else set()
        if live and not op.startswith("s_") and regs(rest) & live:
            bad.append(ins)
        if op.startswith("v_mfma"):
            census["mfma"] += 1
        elif op.startswith("v_"):
            census["valu"] += 1
            census["exp"] += op.startswith("v_exp_f32")
            census["pk"] += op.startswith("v_pk_") and "f32" in op
        elif op.startswith("ds_"):
            tr = op.startswith("ds_read_b64_tr_b16")
            census["tr" if tr else "ds_read" if "read" in op else "ds_write" if "write" in op else "ds_other"] += 1
            flight.append((tr, regs(rest.split(",")[0]) if tr else set()))
        elif op.startswith(("s_load", "s_buffer_load")):
            smem += 1
        elif op.startswith(("global_store", "buffer_store")):
            stores[op] = stores.get(op, 0) + 1
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", rest)
            if m:
                n = int(m.group(1))
                if n == 0:
                    flight, smem = [], 0
                elif smem == 0:
                    flight = flight[len(flight) - n:] if n < len(flight) else flight
    return census, stores, bad


def main():
    rc = 0
    for name, body in kernels(sys.argv[1]):
        census, stores, bad = check(body)
        print(f"{name}: {len(body)} instructions")
        print("  " + ", ".join(f"{k} {v}" for k, v in census.items()) + f"; vector instructions per score {census['valu'] / 128:.1f}")
        print("  stores: " + ", ".join(f"{k} x {v}" for k, v in sorted(stores.items())))
        print(f"  transposed reads named before their wait: {len(bad)}")
        for b in bad[:8]:
            print("    " + b)
        rc |= bool(bad)
    return rc


if __name__ == "__main__":
    sys.exit(main())
