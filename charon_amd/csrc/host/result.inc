// result.inc -- Entry, training data, Result state machine, TSV row formatting (include/result.hpp, include/classify_stats.hpp, include/read_entry.hpp:322-337)
// Part of the single translation unit charon_main.cpp (included inside its anonymous namespace, in order); not a
// stand-alone header.

// ---------------------------------------------------------------------------------------------------
// per-read entry as the host sees it (ReadEntry, include/read_entry.hpp:16-64, minus the bit rows)
// ---------------------------------------------------------------------------------------------------
struct Entry {
    std::string read_id;
    uint32_t length = 0, num_hashes = 0;
    float mean_quality = 0, compression = 0;
    std::vector<uint32_t> counts, unique;
    std::vector<double> prob;
    uint8_t call = 255, conf = 0;
    uint32_t model_version = 0;  // version of the KDE models the device used for prob/call/conf
    std::string row;             // TSV row formatted (in parallel) for model_version; empty if not formatted yet
    std::string rec_id, rec_seq, rec_qual, rec2_id, rec2_seq, rec2_qual;  // only kept when --extract is given
    uint32_t rec_index = 0;      // CHARON_GPU_EXTRACT=1, a flight whose records are formed on the device: the read's index in the flight
    uint32_t row_version = 0;
};

// StatsModel training side (include/classify_stats.hpp:34-114,395-584); the probability/call itself runs on the GPU
struct Training {
    struct Data { bool complete = false, pos_complete = false, neg_complete = false; std::vector<float> pos, neg; };
    std::vector<Data> data;
    std::vector<char> model_ready;
    std::vector<std::vector<float>> k_pos, k_neg;  // current KDE datasets per category (reference iteration order)
    bool ready = false;
    uint32_t version = 0;
    uint16_t num_reads_to_fit;
    float lo_hi_threshold;
    // parametric models (include/classify_stats.hpp:116-208,263-268,289-339): per category {shape, loc, scale} (gamma) or
    // {alpha, beta, -} (beta) of the pos and of the neg distribution
    uint32_t dist = CHN_DIST_KDE;
    std::vector<float> p_pos, p_neg;  // [C][3]

    Training(const DehostArguments &opt, uint32_t C, const chn_model &def) : num_reads_to_fit(opt.num_reads_to_fit), lo_hi_threshold(opt.lo_hi_threshold) {
        data.resize(C); model_ready.assign(C, 0);
        dist = opt.dist == "gamma" ? CHN_DIST_GAMMA : opt.dist == "beta" ? CHN_DIST_BETA : CHN_DIST_KDE;
        for (uint32_t c = 0; c < C; ++c) {
            k_pos.emplace_back(def.pos_data[c], def.pos_data[c] + def.pos_n[c]);
            k_neg.emplace_back(def.neg_data[c], def.neg_data[c] + def.neg_n[c]);
            const float gp[3] = {25.0f, 0.0f, 0.02f}, gn[3] = {10.0f, 0.0f, 0.005f}, bp[3] = {6.0f, 4.0f, 0.0f}, bn[3] = {6.0f, 40.0f, 0.0f};
            for (int j = 0; j < 3; ++j) { p_pos.push_back(dist == CHN_DIST_GAMMA ? gp[j] : bp[j]); p_neg.push_back(dist == CHN_DIST_GAMMA ? gn[j] : bn[j]); }
        }
    }
    // mean / variance of include/classify_stats.hpp:20-32 (double sums of float data; the variance accumulator is narrowed to float each step)
    static double mean_of(const std::vector<float> &v) { double s = 0.0; for (float x : v) s += x; return v.empty() ? 0 : s / v.size(); }
    static double variance_of(const std::vector<float> &v, double mean) {
        double s = 0.0;
        for (float val : v) { const float acc = (float)s; s = acc + ((val - mean) * (val - mean)); }
        return v.size() <= 1 ? 0 : s / (v.size() - 1);
    }
    static void fit_gamma(const std::vector<float> &d, float *q) {  // GammaParams::fit :127-137
        const double mu = mean_of(d), ln_mu = std::log(mu);
        double sum_ln = 0.0;
        for (float n : d) sum_ln += std::log(n);
        const double mean_ln = d.empty() ? 0 : sum_ln / d.size(), s = ln_mu - mean_ln;
        q[0] = (float)((3 - s + std::sqrt((s - 3) * (s - 3) + 24 * s)) / (12 * s));
        q[2] = (float)(mu / q[0]);
    }
    static void fit_beta(const std::vector<float> &d, float *q) {  // BetaParams::fit :171-191
        const double mu = mean_of(d), var = variance_of(d, mu);
        q[0] = (float)(mu * ((mu * (1 - mu) / var) - 1));
        q[1] = (float)((1 - mu) * ((mu * (1 - mu) / var) - 1));
    }
    bool check_status(Data &d) {  // :70-78
        if (d.pos.size() >= num_reads_to_fit) d.pos_complete = true;
        if (d.neg.size() >= num_reads_to_fit) d.neg_complete = true;
        if (d.pos_complete && d.neg_complete) d.complete = true;
        return d.complete;
    }
    bool add_pos(Data &d, float v) { if (d.pos.size() < num_reads_to_fit) d.pos.push_back(v); else check_status(d); return d.complete; }       // :80-90
    bool add_neg(Data &d, float v) { if (d.neg.size() < num_reads_to_fit && v > 0) d.neg.push_back(v); else check_status(d); return d.complete; }  // :92-102
    void train(uint32_t i) {  // Model::train (:358-368) -> train_kde (:341-356; fit() copies the data, h unchanged, no sort) / train_gamma (:289-314) / train_beta (:316-339)
        Data &d = data[i];
        if (dist == CHN_DIST_KDE) {
            if (d.pos_complete) { k_pos[i] = d.pos; ++version; }
            if (d.neg_complete) { k_neg[i] = d.neg; ++version; }
        } else if (dist == CHN_DIST_BETA) {
            if (d.pos_complete) { fit_beta(d.pos, &p_pos[3 * i]); ++version; }
            if (d.neg_complete) { fit_beta(d.neg, &p_neg[3 * i]); ++version; }
        } else {
            if (d.pos_complete) { fit_gamma(d.pos, &p_pos[3 * i]); ++version; }
            if (d.neg_complete) fit_gamma(d.neg, &p_neg[3 * i]);
            else p_neg[3 * i + 1] = (float)(mean_of(d.neg) - (p_neg[3 * i] * p_neg[3 * i + 2]));  // g_neg.fit_loc on the incomplete set (:306-312)
            ++version;
        }
        model_ready[i] = 1;
        d.pos.clear(); d.neg.clear();
    }
    void check_if_ready() { if (ready) return; for (char r : model_ready) if (!r) return; ready = true; }
    void train_model_at(uint32_t i) { train(i); check_if_ready(); }  // :521-533
    void force_ready() { for (uint32_t i = 0; i < data.size(); ++i) if (!model_ready[i]) train(i); ready = true; }  // :463-473
    bool add_read(const std::vector<float> &props) {  // add_read_to_training_data :535-578
        uint8_t pos_i = 255;
        double max_val = 0.0;
        int num_above = 0;
        for (uint8_t i = 0; i < props.size(); ++i) {
            const float val = props[i];
            if (val > lo_hi_threshold) num_above += 1;
            if (val == max_val) pos_i = 255;
            else if (val > max_val) { pos_i = i; max_val = val; }
        }
        const bool to_pos = (pos_i != 255 && num_above == 1);
        const bool to_neg = to_pos || (num_above == 0);
        if (to_pos) { if (add_pos(data[pos_i], props[pos_i]) && !model_ready[pos_i]) train_model_at(pos_i); }
        if (to_neg)
            for (uint8_t i = 0; i < props.size(); ++i)
                if (i != pos_i) { if (add_neg(data[i], props[i]) && !model_ready[i]) train_model_at(i); }
        return ready;
    }
};

struct IndexMeta;
struct Entry;
void format_row(const IndexMeta &meta, const Entry &e, std::string &out);

#define CHN_CHECK(call)                                                                              \
    do {                                                                                             \
        int _rc = (call);                                                                            \
        if (_rc != CHN_OK) throw std::runtime_error(std::string(#call) + " failed: " + chn_last_error()); \
    } while (0)

// CHARON_GPU_DEFLATE=1: the extract files are compressed on the device (chn_deflate_run, BGZF members of 65 280 bytes) instead of by zlib
// on the -t threads; set in main() before anything else runs
bool g_gpu_deflate = false;
int g_gpu_deflate_device = 0;
double g_gpu_deflate_s = 0;  // main-thread seconds inside chn_deflate_run (CHARON_TIMING)
// CHARON_GPU_EXTRACT=1 (with CHARON_GPU_TEXT=1, CHARON_GPU_DEFLATE=1 and --extract): every FASTQ extract file is a chn_extract on the
// device of the resident text.  The records of a flight that is classified at once are formed there out of the flight's text
// (chn_extract_append_records); the bytes the host forms itself -- reads handled while the models train, the host parser's after the
// resident mode was left -- go up through chn_extract_append_bytes, in the order of add_read.  Only BGZF members come down.  The file's
// bytes are those of flush_extract_gpu: its text cut at multiples of CHN_DEFLATE_MAX_IN from its start.  Set in main(); dehost_main
// clears it where it does not apply.
bool g_gpu_extract = false;
uint64_t g_gpu_extract_records = 0, g_gpu_extract_host_bytes = 0, g_gpu_extract_down = 0;  // CHARON_TIMING
double g_gpu_extract_s = 0;  // main-thread seconds inside the chn_extract calls

// Result (include/result.hpp): cache while training, classify, print, count
class Result {
    const IndexMeta &meta_;
    const DehostArguments &opt_;
    chn_stream *stream_;
    chn_model base_model_;
    Training training_;
    std::vector<Entry> cached_;
    size_t cache_capacity_ = 0;
    uint32_t device_model_version_ = 0;
    std::vector<uint64_t> classified_counts_;
    uint64_t unclassified_ = 0;
    std::ostream &out_;
    bool dehost_;  // call_host (single-end) vs call_category (paired; src/dehost_main.cpp:470,475)
    // extract_handles_ (include/result.hpp:44,80-85): one gz FASTA/FASTQ writer per requested category (two when paired)
    // The files are gzip members written back to back (a valid .gz for every reader): records are collected per file and, every 32 MB,
    // cut into pieces at record boundaries that the -t threads deflate side by side (level 6, zlib's default, what gzopen would use).
    // One zlib stream fed record by record -- what a gzFile is -- compresses 27 MB/s: 37 s for the 1 GB that 100 000 extracted 5 kb
    // reads are, whatever else the run does.
    struct ExtractFile {
        FILE *f = nullptr;
        bool fastq = false, wrote = false;
        std::string path, pending;
        std::vector<size_t> cuts;  // record boundaries in `pending`, about 1 MB apart
        chn_extract *gx = nullptr;         // CHARON_GPU_EXTRACT=1: the file on the device, created with the first bytes
        std::vector<uint32_t> picked;      // ... and the reads of the flight at hand that go to this file (Entry::rec_index)
    };
    bool picking_ = false;  // CHARON_GPU_EXTRACT=1: between begin_device_records and append_device_records, extract() notes indices
    std::map<uint8_t, std::vector<ExtractFile>> extract_;
    chn_deflate *deflater_ = nullptr;  // CHARON_GPU_DEFLATE=1: created with the first piece
    std::vector<uint8_t> deflated_;

    static std::string gzip_member(const char *p, size_t n) {
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 31, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2 failed");
        std::string out;
        out.resize(deflateBound(&zs, (uLong)n) + 64);
        zs.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(p)); zs.avail_in = (uInt)n;
        zs.next_out = reinterpret_cast<Bytef *>(&out[0]); zs.avail_out = (uInt)out.size();
        const int rc = deflate(&zs, Z_FINISH);
        const size_t produced = zs.total_out;
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) throw std::runtime_error("deflate failed");
        out.resize(produced);
        return out;
    }
    // CHARON_GPU_DEFLATE=1: the pending bytes in pieces of CHN_DEFLATE_MAX_IN bytes, one BGZF member each (record boundaries do not matter
    // to BGZF), in one chn_deflate_run.  A tail shorter than a piece stays pending unless the file is being closed.
    void flush_extract_gpu(ExtractFile &x, bool closing) {
        const size_t piece = CHN_DEFLATE_MAX_IN, whole = x.pending.size() / piece, take = closing ? x.pending.size() : whole * piece;
        const size_t n = (take + piece - 1) / piece;
        x.cuts.clear();
        if (n == 0) return;
        std::vector<uint64_t> in_off(n), out_off(n);
        std::vector<uint32_t> in_len(n), out_len(n);
        for (size_t i = 0; i < n; ++i) { in_off[i] = i * piece; in_len[i] = (uint32_t)std::min(piece, take - i * piece); }
        uint64_t bound = 0, used = 0;
        bool ok = chn_deflate_bound(n, take, CHN_DEFLATE_BGZF, &bound) == CHN_OK;
        if (ok && !deflater_) ok = chn_deflate_create(g_gpu_deflate_device, &deflater_) == CHN_OK;
        if (ok) {
            if (deflated_.size() < bound) deflated_.resize(bound);
            chn_deflate_job job;
            std::memset(&job, 0, sizeof job);
            job.struct_size = sizeof job; job.flags = CHN_DEFLATE_BGZF; job.n_members = n;
            job.in = reinterpret_cast<const uint8_t *>(x.pending.data()); job.in_bytes = take;
            job.in_offset = in_off.data(); job.in_length = in_len.data();
            job.out = deflated_.data(); job.out_bytes = deflated_.size();
            job.out_offset = out_off.data(); job.out_length = out_len.data(); job.out_used = &used;
            const double t0 = omp_get_wtime();
            ok = chn_deflate_run(deflater_, &job) == CHN_OK;
            g_gpu_deflate_s += omp_get_wtime() - t0;
        }
        if (!ok) throw std::runtime_error("compressing the extract file " + x.path + " failed: " + chn_last_error());
        if (std::fwrite(deflated_.data(), 1, used, x.f) != used) throw std::runtime_error("write to extract file " + x.path + " failed");
        x.wrote = true;
        x.pending.erase(0, take);
    }
    bool on_device(const ExtractFile &x) const { return g_gpu_extract && x.fastq; }
    void gx_write(ExtractFile &x, uint64_t used) {
        g_gpu_extract_down += used;
        if (used && std::fwrite(deflated_.data(), 1, used, x.f) != used) throw std::runtime_error("write to extract file " + x.path + " failed");
        if (used) x.wrote = true;
    }
    // room in deflated_ for what an append of `bytes` (0: chn_extract_finish) may return
    void gx_room(ExtractFile &x, uint64_t bytes) {
        uint64_t bound = 0;
        bool ok = x.gx || chn_extract_create(g_gpu_deflate_device, &x.gx) == CHN_OK;
        ok = ok && chn_extract_bound(x.gx, bytes, &bound) == CHN_OK;
        if (!ok) throw std::runtime_error("compressing the extract file " + x.path + " failed: " + chn_last_error());
        if (deflated_.size() < bound) deflated_.resize(bound);
    }
    // CHARON_GPU_EXTRACT=1: the bytes the host formed, behind everything appended so far
    void flush_extract_gx(ExtractFile &x) {
        x.cuts.clear();
        if (x.pending.empty()) return;
        gx_room(x, x.pending.size());
        uint64_t used = 0;
        const double t0 = omp_get_wtime();
        const bool ok = chn_extract_append_bytes(x.gx, reinterpret_cast<const uint8_t *>(x.pending.data()), x.pending.size(), deflated_.data(), deflated_.size(), &used) == CHN_OK;
        g_gpu_extract_s += omp_get_wtime() - t0;
        if (!ok) throw std::runtime_error("compressing the extract file " + x.path + " failed: " + chn_last_error());
        g_gpu_extract_host_bytes += x.pending.size();
        x.pending.clear();
        gx_write(x, used);
    }
    void flush_extract(ExtractFile &x) {
        if (on_device(x)) { flush_extract_gx(x); return; }
        if (g_gpu_deflate) { flush_extract_gpu(x, false); return; }
        if (x.pending.empty()) return;
        std::vector<size_t> b(1, 0);
        for (size_t c : x.cuts) if (c > b.back() && c < x.pending.size()) b.push_back(c);
        b.push_back(x.pending.size());
        const long pieces = (long)b.size() - 1;
        std::vector<std::string> members((size_t)pieces);
        bool bad = false;
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max<int>(1, opt_.threads))
        for (long i = 0; i < pieces; ++i) {
            try { members[(size_t)i] = gzip_member(x.pending.data() + b[(size_t)i], b[(size_t)i + 1] - b[(size_t)i]); }
            catch (...) {
#pragma omp critical(extract_bad)
                bad = true;
            }
        }
        if (bad) throw std::runtime_error("compressing the extract file " + x.path + " failed");
        for (const std::string &m : members)
            if (std::fwrite(m.data(), 1, m.size(), x.f) != m.size()) throw std::runtime_error("write to extract file " + x.path + " failed");
        x.wrote = true;
        x.pending.clear(); x.cuts.clear();
    }
    void close_extract(ExtractFile &x) {
        if (!x.f) return;
        if (g_gpu_deflate) {  // every file ends with BGZF's end-of-file marker; one that got no record is the marker alone
            if (on_device(x)) {
                flush_extract_gx(x);
                if (x.gx) {
                    gx_room(x, 0);
                    uint64_t used = 0;
                    const double t0 = omp_get_wtime();
                    const bool done = chn_extract_finish(x.gx, deflated_.data(), deflated_.size(), &used) == CHN_OK;
                    g_gpu_extract_s += omp_get_wtime() - t0;
                    if (!done) throw std::runtime_error("compressing the extract file " + x.path + " failed: " + chn_last_error());
                    gx_write(x, used);
                    (void)chn_extract_destroy(x.gx);
                    x.gx = nullptr;
                }
            } else {
                flush_extract_gpu(x, true);
            }
            static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const bool ok = std::fwrite(eof, 1, sizeof eof, x.f) == sizeof eof;
            if (std::fclose(x.f) != 0 || !ok) { x.f = nullptr; throw std::runtime_error("write to extract file " + x.path + " failed"); }
            x.f = nullptr;
            return;
        }
        flush_extract(x);
        if (!x.wrote) { const std::string m = gzip_member("", 0); (void)std::fwrite(m.data(), 1, m.size(), x.f); }  // an empty member, as gzclose writes
        std::fclose(x.f);
        x.f = nullptr;
    }

    // seqan3::sequence_file_output record layout [3P-recall]: FASTQ "@id\nSEQ\n+\nQUAL\n"; FASTA ">id\n" + the sequence in
    // lines of 80 letters.  The sequence is the record's dna5 content, i.e. upper case with every non-ACGT letter as N.
    void write_record(ExtractFile &x, const std::string &id, const std::string &seq, const std::string &qual) {
        std::string &o = x.pending;
        o.reserve(o.size() + id.size() + seq.size() * 2 + 16);
        o += x.fastq ? '@' : '>';
        o += id; o += '\n';
        if (x.fastq) {
            static const struct Up { char t[256]; Up() { for (int c = 0; c < 256; ++c) t[c] = "ACGTN"[g_codes.t[c] & 7]; } } up;
            const size_t at = o.size();
            o.resize(at + seq.size());
            char *dst = &o[at];
            for (size_t i = 0; i < seq.size(); ++i) dst[i] = up.t[(unsigned char)seq[i]];
            o += "\n+\n"; o += qual; o += '\n';
        } else {
            for (size_t i = 0; i < seq.size(); ++i) {
                o += "ACGTN"[g_codes.t[(unsigned char)seq[i]] & 7];
                if ((i + 1) % 80 == 0 || i + 1 == seq.size()) o += '\n';
            }
            if (seq.empty()) o += '\n';
        }
        if (o.size() - (x.cuts.empty() ? 0 : x.cuts.back()) >= ((size_t)1 << 20)) x.cuts.push_back(o.size());
        if (o.size() >= ((size_t)32 << 20)) flush_extract(x);
    }
    void extract(const Entry &e) {  // extract_read / extract_paired_read (include/result.hpp:118-128)
        auto it = extract_.find(e.call);
        if (it == extract_.end()) return;
        if (picking_) {  // the record is formed on the device at the end of the flight
            for (ExtractFile &x : it->second) x.picked.push_back(e.rec_index);
            return;
        }
        write_record(it->second[0], e.rec_id, e.rec_seq, e.rec_qual);
        if (it->second.size() > 1) write_record(it->second[1], e.rec2_id, e.rec2_seq, e.rec2_qual);
    }

    void push_model_to_device() { push_model_to_device(stream_); }

public:
    // the current models to the stream of an index replica (`charon dehost` with CHARON_DEVICES), or to the Result's own stream
    uint32_t push_model_to_device(chn_stream *stream) {
        const uint32_t C = (uint32_t)meta_.categories.size();
        std::vector<const float *> pp(C), np(C);
        std::vector<uint32_t> pn(C), nn(C);
        for (uint32_t c = 0; c < C; ++c) {
            pp[c] = training_.k_pos[c].data(); pn[c] = (uint32_t)training_.k_pos[c].size();
            np[c] = training_.k_neg[c].data(); nn[c] = (uint32_t)training_.k_neg[c].size();
        }
        chn_model m = base_model_;
        m.pos_data = pp.data(); m.pos_n = pn.data(); m.neg_data = np.data(); m.neg_n = nn.data();
        m.dist = training_.dist; m.pos_params = training_.p_pos.data(); m.neg_params = training_.p_neg.data();
        CHN_CHECK(chn_model_set(stream, &m));
        if (stream == stream_) device_model_version_ = training_.version;
        return training_.version;
    }

private:
    // bring prob/call/conf of `es` up to the current models (device K3 on the cached counts)
    void reclassify(std::vector<Entry *> &es) {
        if (es.empty()) return;
        if (device_model_version_ != training_.version) push_model_to_device();
        const size_t C = meta_.categories.size();
        const size_t chunk = (size_t)std::min<uint64_t>(1 << 16, opt_.batch_reads);  // <= the stream's max_reads
        for (size_t b = 0; b < es.size(); b += chunk) {
            const size_t n = std::min(chunk, es.size() - b);
            std::vector<uint32_t> nh(n), cnt(n * C), unq(n * C), len(n);
            std::vector<float> mq(n), comp(n);
            std::vector<double> prob(n * C);
            std::vector<uint8_t> call(n), conf(n);
            for (size_t i = 0; i < n; ++i) {
                const Entry &e = *es[b + i];
                nh[i] = e.num_hashes; len[i] = e.length; mq[i] = e.mean_quality; comp[i] = e.compression;
                for (size_t c = 0; c < C; ++c) { cnt[i * C + c] = e.counts[c]; unq[i * C + c] = e.unique[c]; }
            }
            CHN_CHECK(chn_classify_counts(stream_, n, nh.data(), cnt.data(), unq.data(), len.data(), mq.data(), comp.data(), prob.data(), call.data(), conf.data()));
            for (size_t i = 0; i < n; ++i) {
                Entry &e = *es[b + i];
                e.prob.assign(prob.begin() + i * C, prob.begin() + (i + 1) * C);
                e.call = call[i]; e.conf = conf[i]; e.model_version = training_.version; e.row.clear();
            }
        }
    }
    void print(Entry &e) {  // print_assignment_result, include/read_entry.hpp:322-337
        if (e.row.empty() || e.row_version != e.model_version) { format_row(meta_, e, e.row); e.row_version = e.model_version; }
        out_.write(e.row.data(), (std::streamsize)e.row.size());
    }
    void classify_read(Entry &e) {  // include/result.hpp:97-116
        if (e.model_version != training_.version) { std::vector<Entry *> one(1, &e); reclassify(one); }
        print(e);
        if (e.call < 255) classified_counts_[e.call] += 1; else unclassified_ += 1;
        if (!extract_.empty()) extract(e);  // add_read / classify_cache: extract right after classify_read (:131-136,186-195)
    }
    void classify_cache() {  // :181-198
        std::vector<Entry *> stale;
        for (Entry &e : cached_) if (e.model_version != training_.version) stale.push_back(&e);
        reclassify(stale);
        for (Entry &e : cached_) classify_read(e);
        cached_.clear();
    }

public:
    Result(const IndexMeta &meta, const DehostArguments &opt, chn_stream *stream, const chn_model &base, std::ostream &out)
        : meta_(meta), opt_(opt), stream_(stream), base_model_(base), training_(opt, (uint32_t)meta.categories.size(), base),
          classified_counts_(meta.categories.size(), 0), out_(out), dehost_(!opt.is_paired && !opt.classify_mode) {
        // cached_reads_.reserve() sits inside the `if (opt.run_extract)` loop (include/result.hpp:80-85): capacity 0 otherwise
        if (opt.run_extract) cache_capacity_ = (size_t)opt.num_reads_to_fit * meta.categories.size() * 4;
        for (const auto &kv : opt.extract_category_to_file)
            for (const std::string &path : kv.second) {
                std::string p = path;
                if (ends_with(p, ".gz")) p.resize(p.size() - 3);
                // get_extension (src/utils.cpp:126-133) looks through a trailing .gz only: reads.fastq.bz2 names its extract files
                // <prefix>_<category>.bz2.gz, for which seqan3's sequence_file_output knows no format and throws
                if (ends_with(p, ".bz2")) throw std::runtime_error("cannot tell the sequence format of extract file " + path + " (--extract with .bz2 input: name the reads .fastq/.fasta[.gz])");
                ExtractFile x;
                x.fastq = ends_with(p, ".fastq") || ends_with(p, ".fq");
                x.path = path;
                x.f = std::fopen(path.c_str(), "wb");
                if (!x.f) throw std::runtime_error("cannot create extract file " + path);
                extract_[kv.first].push_back(std::move(x));
            }
    }
    // the stream was created with the default KDE model: a gamma / beta run replaces it before the first batch
    void push_initial_model() { if (training_.dist != CHN_DIST_KDE) push_model_to_device(); }
    ~Result() {
        for (auto &kv : extract_)
            for (ExtractFile &x : kv.second) {
                try { close_extract(x); } catch (...) { if (x.f) std::fclose(x.f); x.f = nullptr; }
                if (x.gx) (void)chn_extract_destroy(x.gx);
            }
        if (deflater_) (void)chn_deflate_destroy(deflater_);
    }
    // CHARON_GPU_EXTRACT=1: the texts and descriptor arrays of a resident flight, by the read's index in the flight; [0] mate 1 / the
    // read, [1] mate 2 (paired input: the second file of a category takes its records from there)
    struct DeviceRecords {
        const uint8_t *text[2] = {nullptr, nullptr};
        uint64_t text_bytes[2] = {0, 0};
        const uint64_t *id_off[2] = {nullptr, nullptr}, *seq_off[2] = {nullptr, nullptr}, *qual_off[2] = {nullptr, nullptr};
        const uint32_t *id_len[2] = {nullptr, nullptr}, *seq_len[2] = {nullptr, nullptr}, *qual_len[2] = {nullptr, nullptr};
    };
    // every add_read up to append_device_records is of a flight whose records are formed on the device (the models are final, so
    // each goes through classify_read at once and in order)
    void begin_device_records() { picking_ = true; }
    void append_device_records(const DeviceRecords &dr) {
        picking_ = false;
        std::vector<uint64_t> o[3];
        std::vector<uint32_t> l[3];
        for (auto &kv : extract_)
            for (size_t m = 0; m < kv.second.size(); ++m) {
                ExtractFile &x = kv.second[m];
                if (x.picked.empty()) continue;
                struct Clear { std::vector<uint32_t> &v; ~Clear() { v.clear(); } } clear{x.picked};
                const size_t k = m ? 1 : 0, n = x.picked.size();
                flush_extract_gx(x);  // what the host formed before this flight comes first
                uint64_t bytes = 0;
                for (int a = 0; a < 3; ++a) { o[a].resize(n); l[a].resize(n); }
                for (size_t i = 0; i < n; ++i) {
                    const uint32_t r = x.picked[i];
                    o[0][i] = dr.id_off[k][r]; l[0][i] = dr.id_len[k][r]; o[1][i] = dr.seq_off[k][r]; l[1][i] = dr.seq_len[k][r];
                    o[2][i] = dr.qual_off[k][r]; l[2][i] = dr.qual_len[k][r];
                    bytes += (uint64_t)l[0][i] + l[1][i] + l[2][i] + 6;
                }
                gx_room(x, bytes);
                chn_extract_job job;
                std::memset(&job, 0, sizeof job);
                job.struct_size = sizeof job; job.text = dr.text[k]; job.text_bytes = dr.text_bytes[k]; job.n_records = n;
                job.id_offset = o[0].data(); job.id_length = l[0].data(); job.seq_offset = o[1].data(); job.seq_length = l[1].data();
                job.qual_offset = o[2].data(); job.qual_length = l[2].data();
                job.out = deflated_.data(); job.out_capacity = deflated_.size();
                const double t0 = omp_get_wtime();
                const bool ok = chn_extract_append_records(x.gx, &job) == CHN_OK;
                g_gpu_extract_s += omp_get_wtime() - t0;
                if (!ok) throw std::runtime_error("forming the records of the extract file " + x.path + " on the device failed: " + chn_last_error());
                g_gpu_extract_records += n;
                gx_write(x, job.out_used);
            }
    }
    Result(const Result &) = delete;
    Result &operator=(const Result &) = delete;
    uint32_t current_model_version() const { return training_.version; }
    void ensure_device_model() { if (device_model_version_ != training_.version) push_model_to_device(); }
    // the models can no longer change (every later read is classified and printed at once, classify_read): batches may then be
    // pipelined and their rows emitted in bulk
    bool models_final() const { return training_.ready; }
    // classify_read for a whole run of reads whose rows were formatted (with the current models) elsewhere: print + count.
    // Only valid when models_final() and nothing is extracted.
    void bulk(const std::string &rows, const std::vector<uint64_t> &per_call /* [C] classified..., [C] = unclassified */) {
        out_.write(rows.data(), (std::streamsize)rows.size());
        for (size_t c = 0; c < classified_counts_.size(); ++c) classified_counts_[c] += per_call[c];
        unclassified_ += per_call[classified_counts_.size()];
    }
    // prob / call / conf of n reads from their counts with the CURRENT models, in one device call (no batch may be in flight)
    void reclassify_raw(size_t n, const uint32_t *nh, const uint32_t *cnt, const uint32_t *unq, const uint32_t *len, const float *mq, const float *comp,
                        double *prob, uint8_t *call, uint8_t *conf) {
        if (device_model_version_ != training_.version) push_model_to_device();
        const size_t C = meta_.categories.size();
        const size_t chunk = (size_t)std::min<uint64_t>(1 << 16, opt_.batch_reads);
        for (size_t b = 0; b < n; b += chunk) {
            const size_t m = std::min(chunk, n - b);
            CHN_CHECK(chn_classify_counts(stream_, m, nh + b, cnt + b * C, unq + b * C, len + b, mq + b, comp + b, prob + b * C, call + b, conf + b));
        }
    }
    // bring entries [from, end) of a batch up to the current models in ONE device call (a model that finishes training in the
    // middle of a batch would otherwise cost a device round trip per remaining read)
    void refresh(std::vector<Entry> &es, size_t from) {
        std::vector<Entry *> stale;
        for (size_t i = from; i < es.size(); ++i) if (es[i].model_version != training_.version) stale.push_back(&es[i]);
        reclassify(stale);
    }

    void add_read(Entry &e) {  // :130-153 (add_paired_read :155-179 differs only in the extract records)
        if (training_.ready) { classify_read(e); return; }
        bool training_complete = false;
        if (cached_.size() < cache_capacity_) {
            cached_.push_back(e);
            std::vector<float> uprops(e.unique.size());
            for (size_t c = 0; c < uprops.size(); ++c) uprops[c] = static_cast<float>(e.unique[c]) / static_cast<float>(e.num_hashes);
            training_complete = training_.add_read(uprops);
        } else {
            training_.force_ready();  // NB: the read that triggers this is dropped, exactly as in the reference
            training_complete = true;
        }
        if (training_complete) classify_cache();
    }
    void complete() {  // :200-202
        classify_cache();
        for (auto &kv : extract_) for (ExtractFile &x : kv.second) close_extract(x);  // (here, not in the destructor: a failed write must be an error)
    }
    void print_summary() {                 // :205-213
        g_log.info("Results summary: ");
        for (size_t i = 0; i < classified_counts_.size(); ++i) g_log.info(meta_.categories[i] + " :\t\t" + std::to_string(classified_counts_[i]));
        g_log.info("unclassified :\t" + std::to_string(unclassified_));
    }
};

std::string first_token(const char *id, uint32_t n) {  // split(id, " ")[0] (src/utils.cpp:9-20)
    const void *sp = std::memchr(id, ' ', n);
    return std::string(id, sp ? (size_t)(static_cast<const char *>(sp) - id) : (size_t)n);
}

// print_assignment_result (include/read_entry.hpp:322-337).  `os << float/double` at precision(6) in the default
// floatfield is printf("%g"); integers as %u.  Formatting rows with snprintf lets batches be formatted in parallel.
// Appends to `out`.
// printf's "%g" (six significant digits, trailing zeros dropped) for the values a row is made of, without printf: most of a row's
// formatting time goes into eight of these.  Exact by construction: for 1e-4 <= |v| < 1e6 the six digits are round-half-even(v * 10^p) with
// p = 5 - floor(log10 |v|); the product is off by at most one part in 10^15, so unless it lands within 1e-6 of a tie (or of a power of ten)
// its rounding is the exact value's rounding.  Everything else -- ties, tiny and huge values, zero's sign, NaN, infinities -- goes to snprintf.
inline size_t format_g6(double v, char *out) {
    const double a = v < 0 ? -v : v;
    if (!(a >= 1e-4 && a < 999999.0)) return (size_t)std::snprintf(out, 32, "%g", v);
    static const double P10[12] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11};
    int X = a >= 1.0 ? (a >= 1e3 ? (a >= 1e5 ? 5 : a >= 1e4 ? 4 : 3) : (a >= 1e2 ? 2 : a >= 1e1 ? 1 : 0)) : (a >= 1e-2 ? (a >= 1e-1 ? -1 : -2) : (a >= 1e-3 ? -3 : -4));
    const int p = 5 - X;                               // digits behind the decimal point: 0 .. 9
    const double scaled = a * P10[p];                  // in [1e5, 1e6) up to rounding
    uint64_t m = (uint64_t)scaled;
    const double frac = scaled - (double)m;
    if (frac > 0.499999 && frac < 0.500001) return (size_t)std::snprintf(out, 32, "%g", v);  // too close to a tie to call here
    if (frac > 0.5) ++m;
    if (m < 100000 || m > 1000000) return (size_t)std::snprintf(out, 32, "%g", v);        // (cannot happen; belt and braces)
    int ndec = p;
    if (m == 1000000) { m = 100000; X += 1; ndec -= 1; if (X >= 6) return (size_t)std::snprintf(out, 32, "%g", v); }
    char d[8];
    for (int i = 5; i >= 0; --i) { d[i] = (char)('0' + m % 10); m /= 10; }
    char *o = out;
    if (v < 0) *o++ = '-';
    if (X >= 0) {
        for (int i = 0; i <= X; ++i) *o++ = d[i];      // integer part: X + 1 digits
        int last = 5;
        while (last > X && d[last] == '0') --last;     // trailing zeros of the fraction go
        if (last > X) { *o++ = '.'; for (int i = X + 1; i <= last; ++i) *o++ = d[i]; }
    } else {
        *o++ = '0'; *o++ = '.';
        for (int i = 0; i < -X - 1; ++i) *o++ = '0';
        int last = 5;
        while (last > 0 && d[last] == '0') --last;
        for (int i = 0; i <= last; ++i) *o++ = d[i];
    }
    (void)ndec;
    *o = 0;
    return (size_t)(o - out);
}
inline size_t format_u32(uint32_t v, char *out) {
    char t[12];
    int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    for (int i = 0; i < n; ++i) out[i] = t[n - 1 - i];
    return (size_t)n;
}

void format_row_raw(const IndexMeta &meta, const char *id, size_t id_len, uint8_t call, uint32_t length, uint32_t num_hashes, float mean_quality,
                    uint8_t conf, float compression, const uint32_t *counts, const uint32_t *unique, const double *prob, std::string &out) {
    char buf[64];
    out += (call == 255 ? "U\t" : "C\t");
    out.append(id, id_len); out += '\t';
    out += meta.category_name(call); out += '\t';
    out.append(buf, format_u32(length, buf)); out += '\t';
    out.append(buf, format_u32(num_hashes, buf)); out += '\t';
    out.append(buf, format_g6((double)mean_quality, buf)); out += '\t';
    out.append(buf, format_u32(conf, buf)); out += '\t';
    out.append(buf, format_g6((double)compression, buf)); out += '\t';
    for (size_t i = 0; i < meta.categories.size(); ++i) {
        const float prop = static_cast<float>(counts[i]) / static_cast<float>(num_hashes);      // get_proportions :140-150
        const float uprop = static_cast<float>(unique[i]) / static_cast<float>(num_hashes);
        out += meta.categories[i];
        out += ':'; out.append(buf, format_u32(counts[i], buf));
        out += ':'; out.append(buf, format_g6((double)prop, buf));
        out += ':'; out.append(buf, format_g6((double)uprop, buf));
        out += ':'; out.append(buf, format_g6(prob[i], buf));
        out += ' ';
    }
    out += '\n';
}
void format_row(const IndexMeta &meta, const Entry &e, std::string &out) {
    out.clear();
    format_row_raw(meta, e.read_id.data(), e.read_id.size(), e.call, e.length, e.num_hashes, e.mean_quality, e.conf, e.compression,
                   e.counts.data(), e.unique.data(), e.prob.data(), out);
}
