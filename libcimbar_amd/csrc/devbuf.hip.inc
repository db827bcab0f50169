// devbuf.hip.inc -- part of cimbar_hip.hip: the owners of everything the host side allocates. Included ONCE, in front of every other section:
// device buffers, page-locked host buffers, events and streams are members of these types, and a context's teardown is its members' destructors.
// None of them synchronises: a caller that replaces a buffer something in flight may still read waits first, itself.
namespace {

// T[capacity] in device memory (PINNED: in page-locked host memory). Move-only; grown on demand, contents NOT preserved.
template <typename T, bool PINNED>
class Buf {
	T* p_ = nullptr;
	size_t cap_ = 0;   // elements

public:
	Buf() = default;
	Buf(const Buf&) = delete;
	Buf& operator=(const Buf&) = delete;
	Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	Buf& operator=(Buf&& o) noexcept { swap(o); return *this; }
	~Buf() { (void)release(); }

	void swap(Buf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
	hipError_t release()
	{
		T* p = p_;
		p_ = nullptr; cap_ = 0;
		if (!p) return hipSuccess;
		if constexpr (PINNED) return hipHostFree(p);
		else return hipFree(p);
	}
	// room for `count` elements: nothing where it has it, else free, then allocate. The capacity is 0 from the first step on, so a failure leaves
	// an empty buffer behind, never a capacity without memory.
	hipError_t reserve(size_t count)
	{
		if (count <= cap_) return hipSuccess;
		if (hipError_t e = release()) return e;
		hipError_t e;
		if constexpr (PINNED) e = hipHostMalloc((void**)&p_, sizeof(T) * count, hipHostMallocDefault);
		else e = hipMalloc((void**)&p_, sizeof(T) * count);
		if (e != hipSuccess) { p_ = nullptr; return e; }
		cap_ = count;
		return hipSuccess;
	}
	// buffers of one fixed size, allocated by whoever needs them first
	hipError_t ensure(size_t count) { return p_ ? hipSuccess : reserve(count); }
	T* get() const { return p_; }
	operator T*() const { return p_; }
	size_t capacity() const { return cap_; }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(const Event&) = delete;
	Event& operator=(const Event&) = delete;
	~Event() { if (e) (void)hipEventDestroy(e); }
	hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
	operator hipEvent_t() const { return e; }
};

struct Stream {
	hipStream_t s = nullptr;
	Stream() = default;
	Stream(const Stream&) = delete;
	Stream& operator=(const Stream&) = delete;
	~Stream() { if (s) (void)hipStreamDestroy(s); }
	hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
	operator hipStream_t() const { return s; }
};

}  // namespace
