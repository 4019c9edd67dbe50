// charstring_decode_support.inc — what the text of the charstring decoder (charstring_decode.inc) stands on: its limits, the reader
// of a stream's bytes and the sink of a glyph's callbacks.  Included, inside their unnamed namespace, by charstring_kernels.hip and
// charstring_batch_kernels.hip behind charstring_kernels.h, charstring_limits.h and include/vgsdf.h.
constexpr int kLanes = 64;
constexpr int kMaxOperands = vg::kCharstringMaxOperands;
constexpr int kMaxOperands2 = vg::kCharstringMaxOperands2;
constexpr int kWindow = vg::kCharstringWindow; // slots of the operand stack in LDS (every slot of the version 1 stamping)
static_assert(kWindow == kMaxOperands, "the version 1 stamping keeps its whole stack in the LDS window");
constexpr int kMaxDepth = vg::kCharstringMaxDepth;
constexpr uint32_t kMaxTokens = VGSDF_CHARSTRING_MAX_TOKENS;

// the stream's bytes through the last word read: a charstring is read front to back, one load per four bytes
struct ByteReader {
	const uint32_t *words;
	uint32_t at = 0xFFFFFFFFu, w = 0;
	__device__ uint32_t u8(uint32_t pos)
	{
		const uint32_t i = pos >> 2;
		if (i != at) {
			at = i;
			w = words[i];
		}
		return (w >> ((pos & 3u) * 8u)) & 0xFFu;
	}
};

// where a glyph's callbacks go: counted, or written into its ranges of kinds / coords
template <bool EMIT> struct Sink {
	uint32_t n_cmds = 0, n_floats = 0;
	uint32_t cmd_room = 0, dat_room = 0; // EMIT: what the count pass found
	uint8_t *kinds = nullptr;
	float *coords = nullptr;
	bool past = false;
	__device__ bool take(uint32_t kind, uint32_t floats)
	{
		if (EMIT) {
			// (once a callback did not fit nothing more is stored: the counters below run on and no longer bound anything)
			if (past || n_cmds >= cmd_room || (uint64_t)n_floats + floats > dat_room) {
				past = true;
				return false;
			}
			kinds[n_cmds] = (uint8_t)kind;
		}
		n_cmds++;
		return true;
	}
	__device__ void point(uint32_t kind, float x, float y)
	{
		if (take(kind, 2) && EMIT) {
			coords[n_floats] = x;
			coords[n_floats + 1] = y;
		}
		n_floats += 2;
	}
	__device__ void move_to(float x, float y) { point(vgsdf::CMD_MOVE, x, y); }
	__device__ void line_to(float x, float y) { point(vgsdf::CMD_LINE, x, y); }
	__device__ void curve_to(float x1, float y1, float x2, float y2, float x, float y)
	{
		if (take(vgsdf::CMD_CURVE, 6) && EMIT) {
			float *c = coords + n_floats;
			c[0] = x1, c[1] = y1, c[2] = x2, c[3] = y2, c[4] = x, c[5] = y;
		}
		n_floats += 6;
	}
	__device__ void close() { (void)take(vgsdf::CMD_CLOSE, 0); }
};
