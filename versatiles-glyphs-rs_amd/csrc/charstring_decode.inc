// charstring_decode.inc — one lane's walk of one glyph id's charstring, the body of charstring_decode (charstring_kernels.hip) and
// of charstring2_batch_decode (charstring_batch_kernels.hip): one text.  EMIT and CFF2 are the including kernel's template
// parameters.  The kernel that includes it names, for a lane that has a glyph id: face (CharstringsRef / Charstrings2Ref), lane
// (of the wave), gid (into face.cs_off and face.fd_of), column (the lane's index in the launch: its column of the workspace), slot
// (EMIT: the glyph id's index into cmd_off / dat_off; else its pair of `counts`), factors_all (CFF2: the factors of the lane's
// position, [n_factors]), counts, cmd_off, dat_off, kinds, coords and flags (one word, the lane's position's).
	__shared__ float stack_lds[kWindow][kLanes];
	__shared__ uint32_t ret_pos[kMaxDepth][kLanes], ret_end[kMaxDepth][kLanes];
	// the operand stack: slot i of this lane (CFF2: past the window, the launch's workspace)
	float *spill = nullptr;
	uint32_t spill_stride = 0;
	if constexpr (CFF2) {
		spill = face.spill + column;
		spill_stride = face.spill_stride;
	}
	auto stk = [&](int i) -> float {
		if constexpr (CFF2) {
			if (i >= kWindow)
				return spill[(size_t)(i - kWindow) * spill_stride];
		}
		return stack_lds[i][lane];
	};
	auto stk_put = [&](int i, float v) {
		if constexpr (CFF2) {
			if (i >= kWindow) {
				spill[(size_t)(i - kWindow) * spill_stride] = v;
				return;
			}
		}
		stack_lds[i][lane] = v;
	};
#define STK(i) stk(i)
	constexpr int kCap = CFF2 ? kMaxOperands2 : kMaxOperands;

	Sink<EMIT> out;
	if (EMIT) {
		const uint32_t c0 = cmd_off[slot], d0 = dat_off[slot];
		out.cmd_room = cmd_off[slot + 1] - c0;
		out.dat_room = dat_off[slot + 1] - d0;
		out.kinds = kinds + c0;
		out.coords = coords + d0;
	}
	ByteReader cs{face.words};
	uint32_t pos = face.cs_off[gid], end = face.cs_off[gid + 1];
	uint32_t fd = 0u; // (CFF2: one set of local subroutines serves every glyph)
	if constexpr (!CFF2)
		fd = face.fd_of ? face.fd_of[gid] : 0u;
	const uint32_t local_first = face.lsubr_first[fd], n_local = face.lsubr_first[fd + 1] - local_first;
	int sp = 0, depth = 0;
	float x = 0.0f, y = 0.0f;
	bool has_move_to = false, first_move_to = true, have_width = CFF2, has_endchar = false;
	uint32_t stems = 0, tokens = 0, raised = 0;
	// CFF2: the factors of the selected set ([n_regions] at `factors`), `vsindex` / `blend` bookkeeping
	const float *factors = nullptr;
	uint32_t n_regions = 0;
	auto select_set = [&](uint32_t set) {
		if constexpr (CFF2) {
			factors = factors_all + face.set_off[set];
			n_regions = face.set_off[set + 1] - face.set_off[set];
		}
	};
	bool had_vsindex = false, had_blend = false;
	if constexpr (CFF2) {
		// set 0 is selected before the first operator: without it the glyph delivers nothing
		if (face.n_sets == 0 || !face.set_ok[0])
			pos = end;
		else
			select_set(0);
	}

	for (;;) {
		if (pos >= end) { // the stream ends: the subroutine (or the charstring) returns
			if (depth == 0)
				break;
			depth--;
			pos = ret_pos[depth][lane];
			end = ret_end[depth][lane];
			if (has_endchar && pos != end)
				break; // data after endchar
			continue;  // (after endchar with pos == end: the caller returns in turn)
		}
		if (++tokens > kMaxTokens) {
			raised |= vgsdf::CS_FLAG_BUDGET;
			break;
		}
		const uint32_t op = cs.u8(pos++);
		if (op >= 32 || op == 28) { // operands
			float v;
			if (op == 28) {
				if (end - pos < 2)
					break;
				v = (float)(int16_t)((cs.u8(pos) << 8) | cs.u8(pos + 1));
				pos += 2;
			} else if (op <= 246) {
				v = (float)((int)op - 139);
			} else if (op <= 250) {
				if (end - pos < 1)
					break;
				v = (float)(((int)op - 247) * 256 + (int)cs.u8(pos) + 108);
				pos += 1;
			} else if (op <= 254) {
				if (end - pos < 1)
					break;
				v = (float)(-((int)op - 251) * 256 - (int)cs.u8(pos) - 108);
				pos += 1;
			} else { // 255: 16.16 fixed
				if (end - pos < 4)
					break;
				const uint32_t b0 = cs.u8(pos), b1 = cs.u8(pos + 1), b2 = cs.u8(pos + 2), b3 = cs.u8(pos + 3);
				v = (float)(int32_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3) / 65536.0f;
				pos += 4;
			}
			if (sp >= kCap)
				break;
			stk_put(sp, v);
			sp++;
			continue;
		}
		bool ok = true; // false: the charstring fails here (the callbacks delivered so far stay)
		if constexpr (CFF2) {
			if (op == 15) { // vsindex: |- ivs vsindex |- , once and before the first blend
				if (had_blend || had_vsindex || sp != 1)
					break;
				const float v = STK(0);
				if (!(v >= 0.0f && v <= 65535.0f))
					break;
				const uint32_t set = (uint32_t)v;
				if (set >= face.n_sets || !face.set_ok[set])
					break;
				select_set(set);
				had_vsindex = true;
				sp = 0;
				continue;
			}
			if (op == 16) { // blend: n values, then their k deltas each, then n; the values stay, each moved by its deltas
				if (sp == 0)
					break;
				had_blend = true;
				const float fn = STK(--sp);
				if (!(fn >= 0.0f && fn <= 65535.0f))
					break;
				const uint32_t n = (uint32_t)fn, k = n_regions; // (n (k + 1) <= 65535 x 65: no overflow)
				const uint32_t len = n * (k + 1);
				if ((uint32_t)sp < len)
					break;
				const int start = sp - (int)len;
				// popped from the top: value n - 1 first, each with its last region's delta first (one product and one sum each)
				for (uint32_t i = n; i-- > 0;) {
					float v = STK(start + (int)i);
					for (uint32_t j = 0; j < k; j++) {
						const float delta = STK(--sp);
						v += delta * factors[k - j - 1];
					}
					stk_put(start + (int)i, v);
				}
				continue;
			}
		}
		switch (op) {
		case 1:  // hstem
		case 3:  // vstem
		case 18: // hstemhm
		case 23: // vstemhm
		{
			int len = sp;
			if ((len & 1) && !have_width) { // an odd count: the first operand is the width
				have_width = true;
				len--;
			}
			stems += (uint32_t)len >> 1;
			sp = 0;
			break;
		}
		case 19: // hintmask
		case 20: // cntrmask
		{
			int len = sp;
			sp = 0;
			if (len & 1) {
				len--;
				have_width = true;
			}
			stems += (uint32_t)len >> 1; // an implied vstem
			const uint32_t mask = (stems + 7) >> 3;
			if (mask > end - pos) {
				if constexpr (CFF2)
					pos = end; // (the stream simply ends; there is no endchar to miss)
				else
					ok = false;
			} else
				pos += mask;
			break;
		}
		case 21: // rmoveto
		case 22: // hmoveto
		case 4:  // vmoveto
		{
			const bool hx = op != 4, hy = op != 22;
			const int want = (hx ? 1 : 0) + (hy ? 1 : 0);
			int skip = 0;
			if (sp == want + 1 && !have_width) {
				skip = 1;
				have_width = true;
			}
			if (sp != skip + want) {
				ok = false;
				break;
			}
			if (first_move_to)
				first_move_to = false;
			else
				out.close();
			has_move_to = true;
			int i = skip;
			if (hx)
				x += STK(i++);
			if (hy)
				y += STK(i++);
			out.move_to(x, y);
			sp = 0;
			break;
		}
		case 5: // rlineto
			if (!has_move_to || (sp & 1)) {
				ok = false;
				break;
			}
			for (int i = 0; i < sp; i += 2) {
				x += STK(i);
				y += STK(i + 1);
				out.line_to(x, y);
			}
			sp = 0;
			break;
		case 6: // hlineto
		case 7: // vlineto
		{
			if (!has_move_to || sp == 0) {
				ok = false;
				break;
			}
			bool horizontal = op == 6;
			for (int i = 0; i < sp; i++) {
				if (horizontal)
					x += STK(i);
				else
					y += STK(i);
				horizontal = !horizontal;
				out.line_to(x, y);
			}
			sp = 0;
			break;
		}
#define CURVE_REL(i)                                                     \
	do {                                                                 \
		const float cx1 = x + STK(i), cy1 = y + STK((i) + 1);            \
		const float cx2 = cx1 + STK((i) + 2), cy2 = cy1 + STK((i) + 3);  \
		x = cx2 + STK((i) + 4);                                          \
		y = cy2 + STK((i) + 5);                                          \
		out.curve_to(cx1, cy1, cx2, cy2, x, y);                          \
	} while (0)
		case 8: // rrcurveto
			if (!has_move_to || sp % 6 != 0) {
				ok = false;
				break;
			}
			for (int i = 0; i < sp; i += 6)
				CURVE_REL(i);
			sp = 0;
			break;
		case 24: // rcurveline
		{
			if (!has_move_to || sp < 8 || (sp - 2) % 6 != 0) {
				ok = false;
				break;
			}
			int i = 0;
			for (; i + 6 <= sp - 2; i += 6)
				CURVE_REL(i);
			x += STK(i);
			y += STK(i + 1);
			out.line_to(x, y);
			sp = 0;
			break;
		}
		case 25: // rlinecurve
		{
			if (!has_move_to || sp < 8 || ((sp - 6) & 1)) {
				ok = false;
				break;
			}
			int i = 0;
			for (; i + 2 <= sp - 6; i += 2) {
				x += STK(i);
				y += STK(i + 1);
				out.line_to(x, y);
			}
			CURVE_REL(i);
			sp = 0;
			break;
		}
		case 26: // vvcurveto
		case 27: // hhcurveto
		{
			if (!has_move_to) {
				ok = false;
				break;
			}
			const bool vv = op == 26;
			int i = 0;
			if (sp & 1) { // (the odd operand is added before the count is checked, as the host reader does)
				if (vv)
					x += STK(0);
				else
					y += STK(0);
				i = 1;
			}
			if ((sp - i) % 4 != 0) {
				ok = false;
				break;
			}
			for (; i < sp; i += 4) {
				if (vv) {
					const float x1 = x, y1 = y + STK(i);
					const float x2 = x1 + STK(i + 1), y2 = y1 + STK(i + 2);
					x = x2;
					y = y2 + STK(i + 3);
					out.curve_to(x1, y1, x2, y2, x, y);
				} else {
					const float x1 = x + STK(i), y1 = y;
					const float x2 = x1 + STK(i + 1), y2 = y1 + STK(i + 2);
					x = x2 + STK(i + 3);
					y = y2;
					out.curve_to(x1, y1, x2, y2, x, y);
				}
			}
			sp = 0;
			break;
		}
		case 30: // vhcurveto
		case 31: // hvcurveto: curves that start horizontal and vertical in turn; the last may carry a fifth operand
		{
			if (!has_move_to || sp < 4) {
				ok = false;
				break;
			}
			bool horizontal = op == 31;
			int i = 0;
			while (i < sp) {
				const int left = sp - i;
				if (left < 4) {
					ok = false;
					break;
				}
				const float last = left == 5 ? STK(i + 4) : 0.0f;
				if (horizontal) {
					const float x1 = x + STK(i), y1 = y;
					const float x2 = x1 + STK(i + 1), y2 = y1 + STK(i + 2);
					y = y2 + STK(i + 3);
					x = x2 + last;
					out.curve_to(x1, y1, x2, y2, x, y);
				} else {
					const float x1 = x, y1 = y + STK(i);
					const float x2 = x1 + STK(i + 1), y2 = y1 + STK(i + 2);
					x = x2 + STK(i + 3);
					y = y2 + last;
					out.curve_to(x1, y1, x2, y2, x, y);
				}
				i += left == 5 ? 5 : 4;
				horizontal = !horizontal;
			}
			sp = 0; // (a failing count leaves the loop with ok == false: the stack no longer matters)
			break;
		}
		case 10: // callsubr
		case 29: // callgsubr
		{
			if (sp == 0 || depth == kMaxDepth) {
				ok = false;
				break;
			}
			const uint32_t n_subrs = op == 29 ? face.n_gsubrs : n_local;
			const float fidx = STK(--sp); // (an operand of a charstring: at most 32768 in magnitude)
			const int idx = (int)fidx + (int)vg::charstring_subr_bias(n_subrs);
			if ((float)(int)fidx != fidx || idx < 0 || idx >= (int)n_subrs) {
				ok = false;
				break;
			}
			const uint32_t *off = op == 29 ? face.gsubr_off + idx : face.lsubr_off + local_first + idx;
			ret_pos[depth][lane] = pos;
			ret_end[depth][lane] = end;
			depth++;
			pos = off[0];
			end = off[1];
			break;
		}
		case 11: // return
			if constexpr (CFF2)
				ok = false; // (not an operator of CFF2: a subroutine ends with its data)
			else
				pos = end;
			break;
		case 14: // endchar
			if constexpr (CFF2) {
				ok = false;
				break;
			}
			if (sp == 4 || (!have_width && sp == 5)) { // the seac form: the charset and two further charstrings — the host's
				raised |= vgsdf::CS_FLAG_SEAC;
				ok = false;
				break;
			}
			if (sp == 1 && !have_width)
				have_width = true;
			sp = 0;
			if (!first_move_to) {
				first_move_to = true;
				out.close();
			}
			if (pos != end) {
				ok = false; // data after endchar
				break;
			}
			has_endchar = true;
			break; // (pos == end: the stream returns at the top of the loop)
		case 12: {
			if (pos >= end) {
				ok = false;
				break;
			}
			const uint32_t op2 = cs.u8(pos++);
			if (!has_move_to) {
				ok = false;
				break;
			}
			if (op2 == 35) { // flex
				if (sp != 13) {
					ok = false;
					break;
				}
				CURVE_REL(0);
				CURVE_REL(6);
			} else if (op2 == 34) { // hflex
				if (sp != 7) {
					ok = false;
					break;
				}
				const float y0 = y;
				float x1 = x + STK(0), y1 = y;
				float x2 = x1 + STK(1), y2 = y1 + STK(2);
				x = x2 + STK(3);
				y = y2;
				out.curve_to(x1, y1, x2, y2, x, y);
				x1 = x + STK(4), y1 = y;
				x2 = x1 + STK(5), y2 = y0;
				x = x2 + STK(6);
				y = y0;
				out.curve_to(x1, y1, x2, y2, x, y);
			} else if (op2 == 36) { // hflex1
				if (sp != 9) {
					ok = false;
					break;
				}
				const float y0 = y;
				float x1 = x + STK(0), y1 = y + STK(1);
				float x2 = x1 + STK(2), y2 = y1 + STK(3);
				x = x2 + STK(4);
				y = y2;
				out.curve_to(x1, y1, x2, y2, x, y);
				x1 = x + STK(5), y1 = y;
				x2 = x1 + STK(6), y2 = y1 + STK(7);
				x = x2 + STK(8);
				y = y0;
				out.curve_to(x1, y1, x2, y2, x, y);
			} else if (op2 == 37) { // flex1
				if (sp != 11) {
					ok = false;
					break;
				}
				const float x0 = x, y0 = y;
				CURVE_REL(0);
				const float x1 = x + STK(6), y1 = y + STK(7);
				const float x2 = x1 + STK(8), y2 = y1 + STK(9);
				if (fabsf(x2 - x0) > fabsf(y2 - y0)) {
					x = x2 + STK(10);
					y = y0;
				} else {
					x = x0;
					y = y2 + STK(10);
				}
				out.curve_to(x1, y1, x2, y2, x, y);
			} else {
				ok = false; // arithmetic, storage and conditional operators: unsupported
				break;
			}
			sp = 0;
			break;
		}
		default:
			ok = false; // 0, 2, 9, 13, 17 (and 15, 16 outside CFF2): reserved
			break;
		}
		if (!ok)
			break;
	}
#undef CURVE_REL
#undef STK
	if (EMIT) {
		if (out.past)
			raised |= vgsdf::CS_FLAG_RANGE;
	} else {
		counts[2 * slot] = out.n_cmds;
		counts[2 * slot + 1] = out.n_floats;
	}
	if (raised)
		atomicOr(flags, raised);
