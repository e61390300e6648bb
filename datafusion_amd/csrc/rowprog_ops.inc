// rowprog_ops.inc — what each RpOp computes, once: the arms `case RP_ADD:` .. `default:` of both interpreters (rowprog.hpp: rp_exec over
// the VGPR register file, tp_exec over the LDS one).  Included INSIDE `switch (in.op)`, after any case the includer keeps to itself
// (rp_exec: RP_LIT; a tile program has no such instruction).  Names in scope at the include:
//   in                  the RpIns (in.aux is read)
//   alo, ahi, an        operand a: 128-bit value and NULL flag          blo, bhi, bn   operand b (whatever the includer fetched for a unary op)
//   olo, ohi, on        the result, preset to 0, 0 and `an | bn`: an arm sets only what differs
// A textual include and not a function: as a function the seven interpreter kernels come out different (profiles/rowprog_one_definition.md).
case RP_ADD: { u128 v = (((u128)ahi << 64) | alo) + (((u128)bhi << 64) | blo); olo = (uint64_t)v; ohi = (uint64_t)(v >> 64); break; }
case RP_SUB: { u128 v = (((u128)ahi << 64) | alo) - (((u128)bhi << 64) | blo); olo = (uint64_t)v; ohi = (uint64_t)(v >> 64); break; }
case RP_MUL: { u128 v = (((u128)ahi << 64) | alo) * (((u128)bhi << 64) | blo); olo = (uint64_t)v; ohi = (uint64_t)(v >> 64); break; }
case RP_SEXT32: { int64_t s = (int64_t)(int32_t)(uint32_t)alo; olo = (uint64_t)s; ohi = (uint64_t)(s >> 63); on = an; break; }
case RP_SEXT64: olo = alo; ohi = (uint64_t)((int64_t)alo >> 63); on = an; break;
case RP_FADD: olo = (uint64_t)__double_as_longlong(__longlong_as_double((long long)alo) + __longlong_as_double((long long)blo)); break;
case RP_FSUB: olo = (uint64_t)__double_as_longlong(__longlong_as_double((long long)alo) - __longlong_as_double((long long)blo)); break;
case RP_FMUL: olo = (uint64_t)__double_as_longlong(__longlong_as_double((long long)alo) * __longlong_as_double((long long)blo)); break;
case RP_I2F: olo = (uint64_t)__double_as_longlong((double)(int64_t)alo); on = an; break;
case RP_F64ORD: { int64_t s = rp_f64_ordered(alo); olo = (uint64_t)s; ohi = (uint64_t)(s >> 63); on = an; break; }
case RP_DATE_PART: { int64_t s = (int64_t)date32_part((int32_t)(uint32_t)alo, (int)in.aux); olo = (uint64_t)s; ohi = (uint64_t)(s >> 63); on = an; break; }
case RP_CMP: olo = rp_cmp128(in.aux, (i128)(((u128)ahi << 64) | alo), (i128)(((u128)bhi << 64) | blo)) ? 1ull : 0ull; break;
case RP_FCMP: olo = rp_cmp128(in.aux, (i128)rp_f64_ordered(alo), (i128)rp_f64_ordered(blo)) ? 1ull : 0ull; break;
case RP_AND: {  // and_kleene: false AND x = false
  bool at = !an && (alo & 1), af = !an && !(alo & 1), bt = !bn && (blo & 1), bf = !bn && !(blo & 1);
  olo = (at && bt) ? 1ull : 0ull;
  on = !((at && bt) || af || bf);
  break;
}
case RP_OR: {  // or_kleene: true OR x = true
  bool at = !an && (alo & 1), af = !an && !(alo & 1), bt = !bn && (blo & 1), bf = !bn && !(blo & 1);
  olo = (at || bt) ? 1ull : 0ull;
  on = !(at || bt || (af && bf));
  break;
}
case RP_NOT: olo = (alo & 1) ^ 1ull; on = an; break;
case RP_IS_NULL: olo = an ? 1ull : 0ull; on = false; break;
case RP_IS_NOT_NULL: olo = an ? 0ull : 1ull; on = false; break;
// b is a non-NULL Boolean: a where it is TRUE, elsewhere a non-NULL 0 (so that MERGE can OR the two gated branches of a CASE together)
case RP_GATE: { const bool g = (blo & 1) != 0; olo = g ? alo : 0ull; ohi = g ? ahi : 0ull; on = g && an; break; }
// at most one side is non-zero / NULL; NULL if either is (the preset `on`)
case RP_MERGE: olo = alo | blo; ohi = ahi | bhi; break;
// a where b is TRUE, NULL where b is FALSE or NULL: unlike GATE, the row drops out of every accumulator
case RP_KEEP_IF: olo = alo; ohi = ahi; on = an || bn || !(blo & 1); break;
default: olo = alo; ohi = ahi; on = an; break;  // RP_MOV
