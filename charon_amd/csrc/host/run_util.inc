// run_util.inc -- the small things every stage of `charon dehost` shares: one clock, one scope guard, one initialiser for the structs of
// the C ABI, the input-error type.  Neither HIP nor Result in here: tools/dehost_pipeline_check.cpp includes it as it stands.
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a stand-alone header.

// seconds on the steady clock (differences are what counts)
inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// runs `fn` when the scope is left, whatever way: auto guard = scope_exit([&] { ... });
template <class Fn>
class ScopeExit {
    Fn fn_;
    bool armed_ = true;

public:
    explicit ScopeExit(Fn fn) : fn_(std::move(fn)) {}
    ScopeExit(ScopeExit &&o) : fn_(std::move(o.fn_)), armed_(o.armed_) { o.armed_ = false; }
    ScopeExit(const ScopeExit &) = delete;
    ScopeExit &operator=(const ScopeExit &) = delete;
    ~ScopeExit() { if (armed_) fn_(); }
};
template <class Fn>
ScopeExit<Fn> scope_exit(Fn fn) { return ScopeExit<Fn>(std::move(fn)); }

// a struct of the C ABI, zeroed, with its struct_size set
template <class T>
T abi_struct() {
    T s;
    std::memset(&s, 0, sizeof s);
    s.struct_size = sizeof s;
    return s;
}

// a fault of the input (as opposed to one of the device or the program): reported without naming the replica that met it
struct InputError : std::runtime_error { using std::runtime_error::runtime_error; };
