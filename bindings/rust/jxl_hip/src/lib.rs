//! Safe host side of the MI355X JPEG XL reconstruction path for jxl-rs.
//!
//! Mirrors `include/jxl_hip.hpp` (the C++ rendering of the same surface, compiled and tested in this repository by
//! `tests/cpp/frame_parity.cc`): every method carries the name of the jxl-rs function whose work it takes over.
//! This crate depends on nothing but `jxl_hip_sys`; the three seams where the `jxl` crate calls it are listed in
//! INTEGRATION.md section 2.  NOT compiled in the build image of this repository (no Rust toolchain there).
use jxl_hip_sys as sys;
use std::ffi::CStr;
use std::os::raw::c_void;

/// `Error::Gpu(..)` payload for jxl-rs' `#[non_exhaustive] enum Error` (jxl/src/error.rs:15-17).
#[derive(Debug, Clone, PartialEq, Eq)]
pub enum HipError {
    InvalidArgument,
    OutOfMemory,
    Device(String),
    BadState,
    /// -> `Error::InvalidVarDCTTransform`
    InvalidTransform,
    /// a valid stream feature outside the device path: the caller keeps the CPU pipeline for this frame
    Unsupported,
    /// -> `Error::InvalidBlockSizeForChromaSubsampling`
    InvalidBlockSize,
    /// -> `Error::HFBlockOutOfBounds`
    BlockOutOfBounds,
    Unknown(i32),
}

pub type Result<T> = std::result::Result<T, HipError>;

fn check(ctx: *const sys::jxlh_ctx, st: sys::jxlh_status) -> Result<()> {
    match st {
        sys::JXLH_OK => Ok(()),
        sys::JXLH_ERR_INVALID_ARGUMENT => Err(HipError::InvalidArgument),
        sys::JXLH_ERR_OUT_OF_MEMORY => Err(HipError::OutOfMemory),
        sys::JXLH_ERR_DEVICE => {
            let msg = if ctx.is_null() {
                String::new()
            } else {
                // SAFETY: jxlh_last_error returns a NUL-terminated string owned by the context
                unsafe { CStr::from_ptr(sys::jxlh_last_error(ctx)) }.to_string_lossy().into_owned()
            };
            Err(HipError::Device(msg))
        }
        sys::JXLH_ERR_BAD_STATE => Err(HipError::BadState),
        sys::JXLH_ERR_INVALID_TRANSFORM => Err(HipError::InvalidTransform),
        sys::JXLH_ERR_UNSUPPORTED => Err(HipError::Unsupported),
        sys::JXLH_ERR_INVALID_BLOCK_SIZE => Err(HipError::InvalidBlockSize),
        sys::JXLH_ERR_BLOCK_OUT_OF_BOUNDS => Err(HipError::BlockOutOfBounds),
        other => Err(HipError::Unknown(other)),
    }
}

/// One device context (one HIP stream for the kernels + one upload stream per decoding thread).
pub struct Context {
    raw: *mut sys::jxlh_ctx,
}
// SAFETY: frame-level calls are made by one thread; jxlh_submit_group* is re-entrant per `slot`
// (include/jxl_hip.h "Conventions"), which is how `submit_*` below are used from the runner's threads.
unsafe impl Send for Context {}
unsafe impl Sync for Context {}

impl Context {
    /// `n_slots` = the JxlParallelRunner's thread count (jxl/src/api/mod.rs:77-81).
    pub fn new(device: i32, n_slots: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        // SAFETY: out pointer is valid
        check(std::ptr::null(), unsafe { sys::jxlh_ctx_create(device, n_slots, &mut raw) })?;
        Ok(Self { raw })
    }
    pub fn raw(&self) -> *mut sys::jxlh_ctx {
        self.raw
    }
    /// `jxlh_stage_save`: the save tail on caller planes in host memory -- `planes` are 3 colour + extra-channel planes of
    /// `w x h` samples at `stride`; `frame_origin` is the position of plane pixel (0, 0) in its frame (the dither table
    /// sees it); `out` holds the whole oriented image at `bytes_per_row`.  What a Modular frame calls.
    #[allow(clippy::too_many_arguments)]
    pub fn stage_save(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc, planes: &[&[f32]], w: u32,
                      h: u32, stride: usize, frame_origin: (u32, u32), y0: u32, y1: u32, out: &mut [u8],
                      bytes_per_row: usize) -> Result<()> {
        if w == 0 || h == 0 || stride < w as usize || !save_fits(desc, w, h, bytes_per_row, out.len()) {
            return Err(HipError::InvalidArgument);
        }
        let need = (h as usize - 1).checked_mul(stride).and_then(|n| n.checked_add(w as usize));
        match need {
            Some(n) if planes.iter().all(|p| p.len() >= n) => {}
            _ => return Err(HipError::InvalidArgument),
        }
        let ptrs: Vec<*const f32> = planes.iter().map(|p| p.as_ptr()).collect();
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        // SAFETY: every plane holds h rows of w samples at `stride`, `out` the whole oriented image; the call waits
        self.ok(unsafe {
            sys::jxlh_stage_save(self.raw, colour, desc, ptrs.as_ptr(), ptrs.len() as u32, w, h, stride, frame_origin.0,
                                 frame_origin.1, y0, y1, out.as_mut_ptr() as *mut c_void, bytes_per_row)
        })
    }
    /// `jxlh_stage_save_rects`: `stage_save` for a list of rectangles of the planes instead of a row band.
    #[allow(clippy::too_many_arguments)]
    pub fn stage_save_rects(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc, planes: &[&[f32]],
                            w: u32, h: u32, stride: usize, frame_origin: (u32, u32), rects: &[sys::save_rects::jxlh_rect],
                            out: &mut [u8], bytes_per_row: usize) -> Result<()> {
        if w == 0 || h == 0 || stride < w as usize || !save_fits(desc, w, h, bytes_per_row, out.len()) {
            return Err(HipError::InvalidArgument);
        }
        let need = (h as usize - 1).checked_mul(stride).and_then(|n| n.checked_add(w as usize));
        match need {
            Some(n) if planes.iter().all(|p| p.len() >= n) => {}
            _ => return Err(HipError::InvalidArgument),
        }
        let ptrs: Vec<*const f32> = planes.iter().map(|p| p.as_ptr()).collect();
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        // SAFETY: every plane holds h rows of w samples at `stride`, `out` the whole oriented image; the call waits
        self.ok(unsafe {
            sys::save_rects::jxlh_stage_save_rects(self.raw, colour, desc, ptrs.as_ptr(), ptrs.len() as u32, w, h, stride,
                                                   frame_origin.0, frame_origin.1, rects.as_ptr(), rects.len() as u32,
                                                   out.as_mut_ptr() as *mut c_void, bytes_per_row)
        })
    }
    /// `jxlh_frame_set_modular_groups`: the group-local transforms of a Modular frame on the device.  `arena` holds
    /// every group's coded channels and palettes (host memory), `groups` each group's rect, transform list in bitstream
    /// order and offsets into the arena (what `decode_modular_section` leaves instead of running `local_apply`).  All
    /// groups run in one launch; the call returns when `arena` may be reused.  A group the device does not take
    /// (`HipError::Unsupported`: delta palettes, local squeeze -- see `set_modular_groups_squeeze`) stays on the host
    /// and goes in with `jxlh_frame_set_modular_channels`.
    pub fn set_modular_groups(&self, arena: &[i32], groups: &[sys::jxlh_local_group], sample_format: u32) -> Result<()> {
        let mut first_bad = usize::MAX;
        // SAFETY: the library checks every offset + extent against arena.len() before it reads; the call waits
        self.ok(unsafe {
            sys::jxlh_frame_set_modular_groups(self.raw, arena.as_ptr(), arena.len() as u64, groups.as_ptr(), groups.len(),
                                               sample_format, &mut first_bad)
        })
    }
    /// `jxlh_modular_local_lower`: the host-side lowering and checks alone; `Err` carries the first refused group
    pub fn lower_modular_groups(groups: &[sys::jxlh_local_group], bit_depth: u32, arena_samples: u64)
                                -> std::result::Result<Vec<sys::jxlh_local_program>, (sys::jxlh_status, usize)> {
        // SAFETY: plain-old-data structs, fully written by a successful call
        let mut progs: Vec<sys::jxlh_local_program> = vec![unsafe { std::mem::zeroed() }; groups.len()];
        let mut first_bad = usize::MAX;
        let st = unsafe {
            sys::jxlh_modular_local_lower(groups.as_ptr(), groups.len(), bit_depth, arena_samples, progs.as_mut_ptr(), &mut first_bad)
        };
        if st == sys::JXLH_OK { Ok(progs) } else { Err((st, first_bad)) }
    }
    /// `jxlh_frame_set_modular_groups_squeeze`: `set_modular_groups` for groups that carry a local squeeze
    /// (`jxl_hip_local_squeeze.h`).  `groups` are self-contained: the steps in front of the squeeze, and ranges of `coded`
    /// (the coded channels in the reference's list order, each with its own size and stride) and of `params` (the
    /// squeeze's `SqueezeParams`; an empty range is `default_squeeze`).  `wp`: one weighted-predictor header per group,
    /// or `None` when no step has predictor 6.  The launches do not grow with the number of groups; the call returns when
    /// `arena` may be reused.
    pub fn set_modular_groups_squeeze(&self, arena: &[i32], groups: &[sys::local_squeeze::jxlh_local_squeeze_group],
                                      coded: &[sys::local_squeeze::jxlh_local_coded_channel],
                                      params: &[sys::local_squeeze::jxlh_squeeze_params], wp: Option<&[sys::jxlh_wp_header]>,
                                      sample_format: u32) -> Result<()> {
        if wp.map_or(false, |w| w.len() != groups.len()) {
            return Err(HipError::InvalidArgument);
        }
        let mut first_bad = usize::MAX;
        // SAFETY: the library checks every range against coded.len() / params.len() and every offset + extent against
        // arena.len() before it reads; the call waits
        self.ok(unsafe {
            sys::local_squeeze::jxlh_frame_set_modular_groups_squeeze(
                self.raw, arena.as_ptr(), arena.len() as u64, groups.as_ptr(), groups.len(), coded.as_ptr(), coded.len(),
                params.as_ptr(), params.len(), wp.map_or(std::ptr::null(), |w| w.as_ptr()), sample_format, &mut first_bad)
        })
    }
    /// `jxlh_frame_set_modular_groups_extra`: `set_modular_groups_squeeze` for groups whose channels are the frame's
    /// colour channels followed by extra channels, or extra channels only (`jxl_hip_local_extra.h`): an RGBA or grey +
    /// alpha image, the alpha / depth / spot channels of a VarDCT frame.  Every finished channel is stored where the
    /// frame keeps it -- colour in the sample planes, channel `n_colour + k` in the sample store of extra channel
    /// `dest.ec[k]`, which must be begun or set -- with the launches of `set_modular_groups_squeeze` and nothing else.
    /// The named extra channels are not rendered until the next run, rerender or repaint.  With `dest.n_colour == 0`
    /// pass `sample_format` 0.  The call returns when `arena` may be reused.
    pub fn set_modular_groups_extra(&self, arena: &[i32], groups: &[sys::local_squeeze::jxlh_local_squeeze_group],
                                    coded: &[sys::local_squeeze::jxlh_local_coded_channel],
                                    params: &[sys::local_squeeze::jxlh_squeeze_params], wp: Option<&[sys::jxlh_wp_header]>,
                                    sample_format: u32, dest: &sys::local_extra::jxlh_local_dest) -> Result<()> {
        if wp.map_or(false, |w| w.len() != groups.len()) {
            return Err(HipError::InvalidArgument);
        }
        let mut first_bad = usize::MAX;
        // SAFETY: as for set_modular_groups_squeeze; `dest` is read before the call returns, and the library checks its
        // channel indices against the frame's extra channels before it stores anything
        self.ok(unsafe {
            sys::local_extra::jxlh_frame_set_modular_groups_extra(
                self.raw, arena.as_ptr(), arena.len() as u64, groups.as_ptr(), groups.len(), coded.as_ptr(), coded.len(),
                params.as_ptr(), params.len(), wp.map_or(std::ptr::null(), |w| w.as_ptr()), sample_format, dest, &mut first_bad)
        })
    }
    /// `jxlh_modular_local_lower_squeeze`: the host-side lowering and checks alone; `Err` carries the first refused group
    pub fn lower_modular_squeeze_groups(groups: &[sys::local_squeeze::jxlh_local_squeeze_group],
                                        coded: &[sys::local_squeeze::jxlh_local_coded_channel],
                                        params: &[sys::local_squeeze::jxlh_squeeze_params], wp: Option<&[sys::jxlh_wp_header]>,
                                        bit_depth: u32, arena_samples: u64)
                                        -> std::result::Result<Vec<sys::local_squeeze::jxlh_local_squeeze_program>, (sys::jxlh_status, usize)> {
        // SAFETY: plain-old-data structs, fully written by a successful call
        let mut progs: Vec<sys::local_squeeze::jxlh_local_squeeze_program> = vec![unsafe { std::mem::zeroed() }; groups.len()];
        let mut first_bad = usize::MAX;
        let st = unsafe {
            sys::local_squeeze::jxlh_modular_local_lower_squeeze(
                groups.as_ptr(), groups.len(), coded.as_ptr(), coded.len(), params.as_ptr(), params.len(),
                wp.map_or(std::ptr::null(), |w| w.as_ptr()), bit_depth, arena_samples, progs.as_mut_ptr(), &mut first_bad)
        };
        if st == sys::JXLH_OK { Ok(progs) } else { Err((st, first_bad)) }
    }
    fn ok(&self, st: sys::jxlh_status) -> Result<()> {
        check(self.raw, st)
    }
    pub fn default_params(xsize: u32, ysize: u32) -> sys::jxlh_frame_params {
        // SAFETY: plain-old-data struct, fully written by the call
        let mut p: sys::jxlh_frame_params = unsafe { std::mem::zeroed() };
        unsafe { sys::jxlh_default_frame_params(&mut p, xsize, ysize) };
        p
    }
    /// blocks until the kernels queued so far are done; reports device-side stream errors
    pub fn sync(&self) -> Result<()> {
        self.ok(unsafe { sys::jxlh_ctx_sync(self.raw) })
    }
    /// a point in the context's stream: everything enqueued so far (`jxlh_ctx_mark`)
    pub fn mark(&self) -> Result<u32> {
        let mut m = 0u32;
        self.ok(unsafe { sys::jxlh_ctx_mark(self.raw, &mut m) })?;
        Ok(m)
    }
    /// blocks until `mark` has been reached -- not for work enqueued after it: a decoder streaming frames through one
    /// context waits for frame i's mark after it has submitted and enqueued frame i + 1
    pub fn wait_mark(&self, mark: u32) -> Result<()> {
        self.ok(unsafe { sys::jxlh_ctx_wait_mark(self.raw, mark) })
    }
    /// Hand-over of device buffers the CALLER filled (jxl_hip.h "STREAM ORDERING OF DEVICE POINTERS"): the context's
    /// streams are non-blocking, so work queued on the NULL stream -- `hipMemset` / `hipMemcpy` of a plane that is then
    /// passed as a device pointer -- is ordered in front of the context's next calls with this.  Call it after the
    /// last fill and before the first entry point that takes the pointer; the host does not block.
    pub fn wait_default_stream(&self) -> Result<()> {
        self.ok(unsafe { sys::jxlh_ctx_wait_stream(self.raw, std::ptr::null_mut()) })
    }
    /// The same for a `hipStream_t` of the caller.
    /// # Safety
    /// `hip_stream` must be a live stream of the context's device.
    pub unsafe fn wait_stream(&self, hip_stream: *mut c_void) -> Result<()> {
        self.ok(sys::jxlh_ctx_wait_stream(self.raw, hip_stream))
    }
    /// ... and for a `hipEvent_t` the caller has recorded behind its fill.
    /// # Safety
    /// `hip_event` must be a live, recorded event.
    pub unsafe fn wait_event(&self, hip_event: *mut c_void) -> Result<()> {
        self.ok(sys::jxlh_ctx_wait_event(self.raw, hip_event))
    }
    /// The other direction: records the caller's event behind everything the context has enqueued on its main stream,
    /// so a caller stream can wait for the results on the device.
    /// # Safety
    /// `hip_event` must be a live event of the context's device.
    pub unsafe fn record_event(&self, hip_event: *mut c_void) -> Result<()> {
        self.ok(sys::jxlh_ctx_record_event(self.raw, hip_event))
    }
    /// pinned host memory for coefficient slabs / pair lists (replaces `VarDctBuffers::coeffs_storage`)
    /// `jxlh_ctx_tune_placement`: the context's next first allocation of its large buffers becomes a pick among `trials`
    /// candidate placements rated on the device (the driver's placement moves the transforms by up to 10 %; setup cost
    /// only, results unchanged).  `trials = 0` only queries.  Returns the last pick's ratings (ms of the two probe
    /// kernels per candidate) and the candidate taken (-1: none yet).
    pub fn tune_placement(&self, trials: i32) -> Result<(Vec<(f32, f32)>, i32)> {
        let mut rep = [0f32; 128];
        let (mut n, mut pick) = (0i32, -1i32);
        check(self.raw, unsafe { sys::jxlh_ctx_tune_placement(self.raw, trials, rep.as_mut_ptr(), rep.len() as i32, &mut n, &mut pick) })?;
        let k = (n.max(0) as usize).min(rep.len()) / 2;
        Ok(((0..k).map(|i| (rep[2 * i], rep[2 * i + 1])).collect(), pick))
    }
    pub fn alloc_pinned(&self, bytes: usize) -> Result<PinnedBuf<'_>> {
        let mut p: *mut c_void = std::ptr::null_mut();
        self.ok(unsafe { sys::jxlh_alloc_pinned(self.raw, bytes, &mut p) })?;
        Ok(PinnedBuf { ctx: self, ptr: p, len: bytes })
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        // SAFETY: created by jxlh_ctx_create, destroyed once
        unsafe { sys::jxlh_ctx_destroy(self.raw) }
    }
}

pub struct PinnedBuf<'a> {
    ctx: &'a Context,
    ptr: *mut c_void,
    len: usize,
}
impl PinnedBuf<'_> {
    pub fn as_mut_slice<T: Copy>(&mut self) -> &mut [T] {
        // SAFETY: hipHostMalloc memory is suitably aligned for any scalar; len is the allocation size
        unsafe { std::slice::from_raw_parts_mut(self.ptr as *mut T, self.len / std::mem::size_of::<T>()) }
    }
    pub fn as_ptr(&self) -> *const c_void {
        self.ptr
    }
}
impl Drop for PinnedBuf<'_> {
    fn drop(&mut self) {
        unsafe { sys::jxlh_free_pinned(self.ctx.raw, self.ptr) };
    }
}

/// `jxlh_changed_rects` (host code, no context): the rectangles of the frame's result, in the frame's coordinates,
/// outside which re-rendering `groups` leaves every pixel as it was -- what `VarDctFrame::save_rects` repaints after a
/// pass.  After `blend`, shift them by the frame's origin in the image and clip them to it.
pub fn changed_rects(params: &sys::jxlh_frame_params, groups: &[u32]) -> Result<Vec<sys::save_rects::jxlh_rect>> {
    let mut n = 0u32;
    // SAFETY: cap = 0 writes no rect; *n is the number needed (the call then reports the missing room)
    let st = unsafe {
        sys::save_rects::jxlh_changed_rects(params, groups.as_ptr(), groups.len() as u32, std::ptr::null_mut(), 0, &mut n)
    };
    if n == 0 {
        return check(std::ptr::null(), st).map(|_| Vec::new());
    }
    let mut rects = vec![sys::save_rects::jxlh_rect { x0: 0, y0: 0, w: 0, h: 0 }; n as usize];
    // SAFETY: `rects` holds the n entries asked for
    check(std::ptr::null(), unsafe {
        sys::save_rects::jxlh_changed_rects(params, groups.as_ptr(), groups.len() as u32, rects.as_mut_ptr(), n, &mut n)
    })?;
    Ok(rects)
}

/// `jxlh_extra_channel_changed_rects` (host code, no context): for rects of new samples of a `w` x `h` extra channel with
/// factor `ec_upsampling`, the rects of the finished channel (cut to `res_w` x `res_h`) outside which every sample is as
/// it was -- one per input rect; what `VarDctFrame::save_rects` repaints, with `changed_rects`, after a pass.
pub fn extra_channel_changed_rects(w: u32, h: u32, ec_upsampling: u32, res_w: u32, res_h: u32,
                                   rects: &[sys::save_rects::jxlh_rect]) -> Result<Vec<sys::save_rects::jxlh_rect>> {
    let mut n = 0u32;
    let mut out = vec![sys::save_rects::jxlh_rect { x0: 0, y0: 0, w: 0, h: 0 }; rects.len()];
    // SAFETY: `out` holds one entry per input rect, which is what the call writes
    check(std::ptr::null(), unsafe {
        sys::extra_rects::jxlh_extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, rects.as_ptr(), rects.len() as u32,
                                                           out.as_mut_ptr(), out.len() as u32, &mut n)
    })?;
    Ok(out)
}

/// `jxlh_blend_image_rects` (host code, no context): rects of a `frame_w` x `frame_h` result -- what `changed_rects`,
/// `repaint_changed_rects` and `extra_channel_changed_rects` return -- as rects of the image `desc` composes the frame
/// onto: shifted by the frame's origin, clipped to the image, empty ones dropped.  The list `VarDctFrame::blend_rects`
/// and, after it, `VarDctFrame::save_rects` take.
pub fn blend_image_rects(desc: &sys::jxlh_blend_desc, frame_w: u32, frame_h: u32,
                         rects: &[sys::save_rects::jxlh_rect]) -> Result<Vec<sys::save_rects::jxlh_rect>> {
    let mut n = 0u32;
    let mut out = vec![sys::save_rects::jxlh_rect { x0: 0, y0: 0, w: 0, h: 0 }; rects.len()];
    // SAFETY: `out` holds one entry per input rect, and the call never writes more than came in
    check(std::ptr::null(), unsafe {
        sys::blend_rects::jxlh_blend_image_rects(desc, frame_w, frame_h, rects.as_ptr(), rects.len() as u32, out.as_mut_ptr(),
                                                 out.len() as u32, &mut n)
    })?;
    out.truncate(n as usize);
    Ok(out)
}

/// A VarDCT frame on the device.  Call order = the reference's frame flow.
pub struct VarDctFrame<'a> {
    ctx: &'a Context,
    pub xsize: u32,
    pub ysize: u32,
    /// size of the frame's own result (the upsampled size of an upsampled frame) and of what the read / save calls see
    /// now: the same, or the image the frame was blended onto
    frame_out: (u32, u32),
    out_size: std::cell::Cell<(u32, u32)>,
}

/// Bytes of one pixel of a save: samples per pixel times the sample size of `format`.
fn save_pixel_bytes(desc: &sys::jxlh_save_desc) -> usize {
    let sample = match desc.format {
        sys::JXLH_SAVE_U8 => 1,
        sys::JXLH_SAVE_F32 => 4,
        _ => 2,
    };
    (desc.n_channels as usize + usize::from(desc.fill_opaque_alpha != 0)) * sample
}

/// Whether `len` bytes hold the oriented image of a `w x h` source at `bytes_per_row`.
fn save_fits(desc: &sys::jxlh_save_desc, w: u32, h: u32, bytes_per_row: usize, len: usize) -> bool {
    let (ow, oh) = if desc.orientation >= 5 { (h as usize, w as usize) } else { (w as usize, h as usize) };
    if ow == 0 || oh == 0 {
        return false;
    }
    let row = match ow.checked_mul(save_pixel_bytes(desc)) {
        Some(r) => r,
        None => return false,
    };
    match (oh - 1).checked_mul(bytes_per_row).and_then(|b| b.checked_add(row)) {
        Some(need) => bytes_per_row >= row && len >= need,
        None => false,
    }
}

impl<'a> VarDctFrame<'a> {
    /// `Frame::from_header_and_toc` + `prepare_render_pipeline` (frame/decode.rs:172-204, frame/render.rs:907)
    pub fn begin(ctx: &'a Context, p: &sys::jxlh_frame_params) -> Result<Self> {
        ctx.ok(unsafe { sys::jxlh_frame_begin(ctx.raw, p) })?;
        let n = p.upsampling.max(1);
        let out = (if p.xsize_upsampled != 0 { p.xsize_upsampled } else { p.xsize * n },
                   if p.ysize_upsampled != 0 { p.ysize_upsampled } else { p.ysize * n });
        Ok(Self { ctx, xsize: p.xsize, ysize: p.ysize, frame_out: out, out_size: std::cell::Cell::new(out) })
    }
    /// `decode_hf_global`: `DequantMatrices::matrix(table, c)` for the 17 tables (frame/quant_weights.rs:1081-1086)
    pub fn decode_hf_global(&self, tables: &[&[f32]; 17]) -> Result<()> {
        let ptrs: Vec<*const f32> = tables.iter().map(|t| t.as_ptr()).collect();
        let n: Vec<usize> = tables.iter().map(|t| t.len() / 3).collect();
        self.ctx.ok(unsafe { sys::jxlh_frame_set_dequant_tables(self.ctx.raw, ptrs.as_ptr(), n.as_ptr()) })
    }
    /// `decode_lf_group` -> `dequant_lf` (frame/modular/mod.rs:837-929): rect in blocks, channels in coded order Y, X, B
    #[allow(clippy::too_many_arguments)]
    pub fn decode_lf_group(&self, x0: u32, y0: u32, w: u32, h: u32, qy: &[i32], qx: &[i32], qb: &[i32], stride: usize,
                           extra_precision: u32) -> Result<()> {
        if w == 0 || h == 0 || stride < w as usize {
            return Err(HipError::InvalidArgument);
        }
        let need = (h as usize - 1) * stride + w as usize;
        if qy.len() < need || qx.len() < need || qb.len() < need {
            return Err(HipError::InvalidArgument);
        }
        self.ctx.ok(unsafe {
            sys::jxlh_frame_set_lf_quantized(self.ctx.raw, x0, y0, w, h, qy.as_ptr(), qx.as_ptr(), qb.as_ptr(), stride,
                                             extra_precision)
        })
    }
    /// `decode_hf_metadata` (frame/modular/mod.rs:984-1081): HfMetadata maps of a rect in blocks
    #[allow(clippy::too_many_arguments)]
    pub fn decode_hf_metadata(&self, x0: u32, y0: u32, w: u32, h: u32, transform_map: &[u8], raw_quant: &[i32],
                              epf_map: &[u8], map_stride: usize, ytox: &[i8], ytob: &[i8], cmap_stride: usize) -> Result<()> {
        // the C side reads h rows of w entries at map_stride, and one colour-tile entry per 8 x 8 blocks
        if w == 0 || h == 0 || map_stride < w as usize || cmap_stride < (w as usize).div_ceil(8) {
            return Err(HipError::InvalidArgument);
        }
        let need = (h as usize - 1) * map_stride + w as usize;
        let cneed = ((h as usize).div_ceil(8) - 1) * cmap_stride + (w as usize).div_ceil(8);
        if transform_map.len() < need || raw_quant.len() < need || epf_map.len() < need || ytox.len() < cneed
            || ytob.len() < cneed {
            return Err(HipError::InvalidArgument);
        }
        self.ctx.ok(unsafe {
            sys::jxlh_frame_set_hf_meta(self.ctx.raw, x0, y0, w, h, transform_map.as_ptr(), raw_quant.as_ptr(),
                                        epf_map.as_ptr(), map_stride, ytox.as_ptr(), ytob.as_ptr(), cmap_stride)
        })
    }
    /// the `if let Some(pixels)` branch of `decode_vardct_group` (frame/group.rs:579-611): the group's dense slab,
    /// 3 x 65536 i32 in pinned memory; asynchronous, reuse the slab after `slot_wait`.  `complete = false` is a
    /// progressive pass whose coefficients will be added to by later passes (`set_buffer_for_group(.., complete, ..)`).
    ///
    /// # Safety
    /// The copy is asynchronous: `coeffs` must stay alive and unmodified until `slot_wait(slot)` has returned (the
    /// borrow this call holds ends when it returns, the device still reads the slab).
    pub unsafe fn decode_vardct_group(&self, slot: i32, group: u32, coeffs: &[i32], complete: bool) -> Result<()> {
        if coeffs.len() != 3 * 65536 {
            return Err(HipError::InvalidArgument);
        }
        let flags = if complete { sys::JXLH_GROUP_COMPLETE } else { 0 };
        self.ctx.ok(sys::jxlh_submit_group(self.ctx.raw, slot, group, coeffs.as_ptr(), flags))
    }
    /// the same from the entropy loop's updates (frame/group.rs:557-572 emits `(position, value)` instead of
    /// `coeffs[position] += value`): `pairs` = X run, Y run, B run
    ///
    /// # Safety
    /// Asynchronous like `decode_vardct_group`: `pairs` and `wide` must stay alive and unmodified until
    /// `slot_wait(slot)` has returned.
    pub unsafe fn decode_vardct_group_sparse(&self, slot: i32, group: u32, pairs: &[sys::jxlh_coeff16], n: [u32; 3],
                                      wide: &[sys::jxlh_coeff32], complete: bool) -> Result<()> {
        if pairs.len() != (n[0] + n[1] + n[2]) as usize {
            return Err(HipError::InvalidArgument);
        }
        let flags = if complete { sys::JXLH_GROUP_COMPLETE } else { 0 };
        self.ctx.ok(sys::jxlh_submit_group_sparse(self.ctx.raw, slot, group, pairs.as_ptr(), n.as_ptr(), wide.as_ptr(),
                                                  wide.len() as u32, flags))
    }
    pub fn slot_wait(&self, slot: i32) -> Result<()> {
        self.ctx.ok(unsafe { sys::jxlh_slot_wait(self.ctx.raw, slot) })
    }
    /// `Frame::finalize_lf` + `SigmaSource::new` + the reconstruction of every submitted group + the Gaborish / EPF
    /// stages of frame/render.rs:569-622 (and chroma upsampling / upsampling / noise when the parameters ask for them)
    pub fn finalize_and_render(&self) -> Result<()> {
        self.out_size.set(self.frame_out); // a render discards a composition
        self.ctx.ok(unsafe { sys::jxlh_frame_run(self.ctx.raw, 0, u32::MAX) })
    }
    /// The colour stage (`None`: the planes are in the output colour space already), `BlendingStage` and
    /// `ExtendToImageDimensionsStage` (frame/render.rs:754-771): the rendered frame composed onto the
    /// `image_w x image_h` image from the context's reference slots.  The image becomes what the read calls and
    /// `jxlh_frame_save_reference` see, until the next render.
    pub fn blend(&self, desc: &sys::jxlh_blend_desc, colour: Option<&sys::jxlh_output_desc>) -> Result<()> {
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        self.ctx.ok(unsafe { sys::jxlh_frame_blend(self.ctx.raw, desc, colour) })?;
        self.out_size.set((desc.image_w, desc.image_h));
        Ok(())
    }
    /// After a re-render of a frame `blend` has composed: only the listed rectangles of the IMAGE (`blend_image_rects`)
    /// are composed again, in the canvas `blend` left (`jxlh_frame_blend_rects`); the image is the frame's result again.
    /// Same descriptor and colour stage as the `blend`.  The caller's contract: every image pixel an input of which
    /// changed since the canvas was last written lies in a rect -- a pixel left out keeps its old value.
    pub fn blend_rects(&self, desc: &sys::jxlh_blend_desc, colour: Option<&sys::jxlh_output_desc>,
                       rects: &[sys::save_rects::jxlh_rect]) -> Result<()> {
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        // SAFETY: `rects` is a live slice of rects.len() entries; the call reads it before it returns
        self.ctx.ok(unsafe {
            sys::blend_rects::jxlh_frame_blend_rects(self.ctx.raw, desc, colour, rects.as_ptr(), rects.len() as u32)
        })?;
        self.out_size.set((desc.image_w, desc.image_h));
        Ok(())
    }
    /// (width, height) of what the read and save calls see: the frame, its upsampled image, or the image it was blended
    /// onto
    pub fn out_size(&self) -> (u32, u32) {
        self.out_size.get()
    }
    /// The save tail of frame/render.rs:793-903 in one pass over the frame's result: spot colours, premultiplication,
    /// the conversion to u8 / u16 / f16 / f32 and the save stage with its channel order, endianness, opaque-alpha fill and
    /// orientation, behind the colour stage `colour` (`None` after `blend`).  Source rows `[y0, y1)` (`y1` is cut at the
    /// result's height) go to their display positions in the whole oriented image at `out`.
    ///
    /// # Safety
    /// `out` must be writable memory (host or device) holding the WHOLE oriented image at `bytes_per_row`: the result's
    /// height in rows for orientations 1-4, its width in rows for 5-8 (the result is the frame, its upsampled image, or
    /// the image it was blended onto -- a size only the caller's headers know).
    pub unsafe fn save(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc, y0: u32, y1: u32,
                       out: *mut c_void, bytes_per_row: usize) -> Result<()> {
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        self.ctx.ok(sys::jxlh_frame_save(self.ctx.raw, colour, desc, y0, y1, out, bytes_per_row))
    }
    /// `save` into host memory, checked: `out` must hold the whole oriented image of the current result (`out_size()`,
    /// transposed for orientations 5-8) at `bytes_per_row`; the call returns after the copy has completed.
    pub fn save_to_slice(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc, y0: u32, y1: u32,
                         out: &mut [u8], bytes_per_row: usize) -> Result<()> {
        let (w, h) = self.out_size.get();
        if !save_fits(desc, w, h, bytes_per_row, out.len()) {
            return Err(HipError::InvalidArgument);
        }
        // SAFETY: the slice holds every byte the oriented image can touch, and the call waits for the copy
        unsafe { self.save(colour, desc, y0, y1, out.as_mut_ptr() as *mut c_void, bytes_per_row) }
    }
    /// `save` without the final wait (`jxlh_frame_save_async`): `out` holds the image after the next `Context::sync`.
    ///
    /// # Safety
    /// As `save`; in addition `out` (pinned host memory, or device memory) must stay valid and untouched until the
    /// context has been synchronised.
    pub unsafe fn save_async(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc, y0: u32, y1: u32,
                             out: *mut c_void, bytes_per_row: usize) -> Result<()> {
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        self.ctx.ok(sys::jxlh_frame_save_async(self.ctx.raw, colour, desc, y0, y1, out, bytes_per_row))
    }
    /// `save` for a list of rectangles of the result instead of a row band (`jxlh_frame_save_rects`): only the pixels
    /// inside a rect (cut at the result's edge) are written, each at its display position in the whole oriented image at
    /// `out`, with the samples `save` gives them; a device destination in one launch, a host destination with one copy
    /// of exactly its pixel bytes per rect.
    ///
    /// # Safety
    /// As `save`.
    pub unsafe fn save_rects(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc,
                             rects: &[sys::save_rects::jxlh_rect], out: *mut c_void, bytes_per_row: usize) -> Result<()> {
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        self.ctx.ok(sys::save_rects::jxlh_frame_save_rects(self.ctx.raw, colour, desc, rects.as_ptr(), rects.len() as u32, out,
                                                           bytes_per_row))
    }
    /// `save_rects` into host memory, checked as `save_to_slice` is; returns after the copies have completed.
    pub fn save_rects_to_slice(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc,
                               rects: &[sys::save_rects::jxlh_rect], out: &mut [u8], bytes_per_row: usize) -> Result<()> {
        let (w, h) = self.out_size.get();
        if !save_fits(desc, w, h, bytes_per_row, out.len()) {
            return Err(HipError::InvalidArgument);
        }
        // SAFETY: the slice holds every byte the oriented image can touch, and the call waits for the copies
        unsafe { self.save_rects(colour, desc, rects, out.as_mut_ptr() as *mut c_void, bytes_per_row) }
    }
    /// `save_rects` without the final wait (`jxlh_frame_save_rects_async`).
    ///
    /// # Safety
    /// As `save_async`.
    pub unsafe fn save_rects_async(&self, colour: Option<&sys::jxlh_output_desc>, desc: &sys::jxlh_save_desc,
                                   rects: &[sys::save_rects::jxlh_rect], out: *mut c_void, bytes_per_row: usize) -> Result<()> {
        let colour = colour.map_or(std::ptr::null(), |c| c as *const sys::jxlh_output_desc);
        self.ctx.ok(sys::save_rects::jxlh_frame_save_rects_async(self.ctx.raw, colour, desc, rects.as_ptr(),
                                                                 rects.len() as u32, out, bytes_per_row))
    }
    /// `mark_group_to_rerender` + re-render (render/mod.rs:143-146): after more passes arrived for `groups`
    pub fn rerender_groups(&self, groups: &[u32]) -> Result<()> {
        self.out_size.set(self.frame_out); // a render discards a composition
        self.ctx.ok(unsafe { sys::jxlh_frame_rerender_groups(self.ctx.raw, groups.as_ptr(), groups.len() as u32) })
    }
    /// `upsample_lf_group` (frame/decode.rs:51-158, taken at :744-752): `group` has no HF yet -- the next render fills it
    /// from the LF image upsampled 8x instead of transforming it; a later submission of the group clears the mark
    pub fn upsample_lf_group(&self, group: u32) -> Result<()> {
        self.ctx.ok(unsafe { sys::jxlh_frame_set_groups_lf_only(self.ctx.raw, &group, 1) })
    }
    /// the save stage for planar f32 XYB output; `out[c]` = `RawImageBuffer` of channel c
    ///
    /// # Safety
    /// Every `out[c]` must describe writable memory (host or device) of `num_rows` rows of `bytes_per_row` bytes at
    /// `bytes_between_rows`: the descriptors carry raw pointers the compiler cannot check.
    pub unsafe fn read_planes(&self, out: &[sys::jxlh_plane; 3]) -> Result<()> {
        self.ctx.ok(sys::jxlh_frame_read_planes(self.ctx.raw, out.as_ptr()))
    }
    /// One 256 x 256 group of the finished planes, the unit `RenderPipeline::set_buffer_for_group` moves
    /// (render/mod.rs:124-137): `out[c]` = the `RawImageBuffer` of the `Image<f32>` `pipeline.get_buffer::<f32>(c)`
    /// returned (the group's size rounded up to 16 pixels, render/internal.rs:144-167).  `xgroups` =
    /// `frame_header.size_groups().0`.  Pixels beyond the frame's edge are left untouched.
    ///
    /// # Safety
    /// See `read_planes`.
    pub unsafe fn read_group_planes(&self, group: u32, xgroups: u32, out: &[sys::jxlh_plane; 3]) -> Result<()> {
        if xgroups == 0 {
            return Err(HipError::InvalidArgument);
        }
        let (x0, y0) = ((group % xgroups) * sys::JXLH_GROUP_DIM, (group / xgroups) * sys::JXLH_GROUP_DIM);
        self.ctx.ok(sys::jxlh_frame_read_planes_rect(self.ctx.raw, x0, y0, sys::JXLH_GROUP_DIM, sys::JXLH_GROUP_DIM,
                                                     out.as_ptr()))
    }
    /// An extra channel as the Modular decoder leaves it (channel 3 + `ec` of the reference's pipeline): `samples` = `h`
    /// rows of `w` i32 at `stride`.  The next `finalize_and_render` applies `ConvertModularToF32Stage::new(3 + ec,
    /// bits_per_sample)` and, for `ec_upsampling` 2 / 4 / 8, the channel's own `Upsample{2,4,8}x` (frame/render.rs:564-567,
    /// :624-637).  The samples are copied before the call returns.
    pub fn set_extra_channel(&self, ec: u32, samples: &[i32], stride: usize, w: u32, h: u32, bits_per_sample: u32,
                             ec_upsampling: u32) -> Result<()> {
        if w == 0 || h == 0 || stride < w as usize || samples.len() < (h as usize - 1) * stride + w as usize {
            return Err(HipError::InvalidArgument);
        }
        self.ctx.ok(unsafe {
            sys::jxlh_frame_set_extra_channel(self.ctx.raw, ec, samples.as_ptr(), stride, w, h, bits_per_sample, ec_upsampling)
        })
    }
    /// An extra channel that arrives group by group (`jxlh_frame_begin_extra_channel`): declared once per frame with
    /// no samples yet -- every sample reads as zero until `set_extra_channel_rects` sets it.
    pub fn begin_extra_channel(&self, ec: u32, w: u32, h: u32, bits_per_sample: u32, ec_upsampling: u32) -> Result<()> {
        self.ctx.ok(unsafe { sys::extra_rects::jxlh_frame_begin_extra_channel(self.ctx.raw, ec, w, h, bits_per_sample, ec_upsampling) })
    }
    /// The samples of extra channels as their groups arrive (`jxlh_frame_set_extra_channel_rects`): every rect names
    /// `h` rows of `w` samples of the host block `samples`, `stride` apart from `offset`, and where they go in channel
    /// `ec`.  One copy and one launch per call; the next `finalize_and_render` / `rerender_groups` converts and
    /// upsamples only what the rects can have changed.  The block is copied before the call returns; a refusal names
    /// the rect in the context's last error.
    pub fn set_extra_channel_rects(&self, samples: &[i32], rects: &[sys::extra_rects::jxlh_ec_rect]) -> Result<()> {
        let mut bad = 0u32;
        self.ctx.ok(unsafe {
            sys::extra_rects::jxlh_frame_set_extra_channel_rects(self.ctx.raw, samples.as_ptr(), samples.len() as u64,
                                                                 rects.as_ptr(), rects.len() as u32, &mut bad)
        })
    }
    /// the save stage of an extra channel: one f32 plane of the frame's output size
    ///
    /// # Safety
    /// `out` must describe writable memory (host or device), see `read_planes`.
    pub unsafe fn read_extra_channel(&self, ec: u32, out: &sys::jxlh_plane) -> Result<()> {
        self.ctx.ok(sys::jxlh_frame_read_extra_channel(self.ctx.raw, ec, out))
    }
    /// XybStage + FromLinearStage(sRGB) + ConvertF32ToU8Stage, interleaved, rows [y0, y1)
    pub fn read_rgb8(&self, p: &sys::jxlh_xyb_params, channels: u32, y0: u32, y1: u32, out: &mut [u8],
                     bytes_per_row: usize) -> Result<()> {
        let rows = y1.checked_sub(y0).ok_or(HipError::InvalidArgument)? as usize;
        if out.len() < rows * bytes_per_row {
            return Err(HipError::InvalidArgument);
        }
        self.ctx.ok(unsafe {
            sys::jxlh_frame_read_rgb8(self.ctx.raw, p, channels, y0, y1, out.as_mut_ptr() as *mut c_void, bytes_per_row)
        })
    }
}

/// The slot-bucketed coefficient form written by the entropy loop itself (`jxlh_slot_writer_*`, include/jxl_hip.h):
/// `current_coeffs[coeff_index] += coeff` of `decode_vardct_group` (jxl/src/frame/group.rs:557-575) becomes `add`, a
/// varblock's start (`coeffs_offset`, `cx * cy`: group.rs:612) `begin_varblock`.  One writer per runner thread.  Values
/// beyond the entry's range are split into repeated in-range entries (they add up on the device); only what no slot can
/// hold lands in `wide`.  Plain CPU code: no context, no device.
pub struct SlotWriter {
    raw: *mut sys::jxlh_slot_writer,
}
// SAFETY: a writer is used by one thread at a time (it holds no thread-affine state)
unsafe impl Send for SlotWriter {}

impl SlotWriter {
    pub fn new() -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(std::ptr::null(), unsafe { sys::jxlh_slot_writer_create(&mut raw) })?;
        Ok(Self { raw })
    }
    /// `entries` (u16 each; room for the group's updates incl. split values), `slot_counts` (3 x 1024, zeroed by the
    /// call) and `wide` are the buffers `jxlh_submit_groups_slots` will read -- typically slices of pinned memory.
    pub fn begin_group(&mut self, group_id: u32, entries: &mut [u16], slot_counts: &mut [u8; 3 * 1024],
                       wide: &mut [sys::jxlh_coeff32]) -> Result<()> {
        check(std::ptr::null(), unsafe {
            sys::jxlh_slot_writer_begin_group(self.raw, group_id, 0, entries.as_mut_ptr() as *mut c_void, entries.len(),
                                              slot_counts.as_mut_ptr(), wide.as_mut_ptr(), wide.len() as u32)
        })
    }
    /// `first_slot` = `coeffs_offset / 64`, `num_slots` = `cx * cy`; varblocks in decode order
    pub fn begin_varblock(&mut self, first_slot: u32, num_slots: u32) -> Result<()> {
        check(std::ptr::null(), unsafe { sys::jxlh_slot_writer_begin_varblock(self.raw, first_slot, num_slots) })
    }
    /// `coeffs[channel][coeffs_offset + pos] += value`
    #[inline]
    pub fn add(&mut self, channel: u32, pos: u32, value: i32) -> Result<()> {
        check(std::ptr::null(), unsafe { sys::jxlh_slot_writer_add(self.raw, channel, pos, value) })
    }
    /// closes the group: entries per channel (the `n` of `jxlh_submit_groups_slots`) and the number of `wide` values
    pub fn end_group(&mut self) -> Result<([u32; 3], u32)> {
        let mut n = [0u32; 3];
        let mut nw = 0u32;
        check(std::ptr::null(), unsafe { sys::jxlh_slot_writer_end_group(self.raw, n.as_mut_ptr(), &mut nw) })?;
        Ok((n, nw))
    }
}

impl Drop for SlotWriter {
    fn drop(&mut self) {
        // SAFETY: created by jxlh_slot_writer_create, destroyed once
        unsafe { sys::jxlh_slot_writer_destroy(self.raw) }
    }
}

/// Dense group slabs -> the arrays of ONE `jxlh_submit_groups_slots` call (`jxlh_host_pack_slots_many`): for a decoder
/// that keeps the reference's per-group `Vec<i32>` (`Frame::hf_coefficients`, jxl/src/frame/mod.rs; 3 x 65536 each).
/// `entries` (u16 each), `slot_counts` (groups x 3 x 1024) and `n` (groups x 3) are written group after group.  Returns
/// (entries written, `wide` values).  Plain CPU code, any thread: each runner thread packs its share of the frame.
pub fn pack_group_slabs(group_coeffs: &[&[i32]], group_ids: &[u32], entries: &mut [u16], slot_counts: &mut [u8],
                        n: &mut [u32], wide: &mut [sys::jxlh_coeff32]) -> Result<(usize, u32)> {
    let k = group_coeffs.len();
    if group_ids.len() != k || slot_counts.len() < k * 3 * 1024 || n.len() < k * 3 || group_coeffs.iter().any(|g| g.len() != 3 * 65536) {
        return Err(HipError::InvalidArgument);
    }
    let ptrs: Vec<*const i32> = group_coeffs.iter().map(|g| g.as_ptr()).collect();
    let (mut nw, mut used) = (0u32, 0usize);
    check(std::ptr::null(), unsafe {
        sys::jxlh_host_pack_slots_many(ptrs.as_ptr(), group_ids.as_ptr(), k as u32, 0, entries.as_mut_ptr() as *mut c_void,
                                       entries.len(), slot_counts.as_mut_ptr(), n.as_mut_ptr(), wide.as_mut_ptr(),
                                       wide.len() as u32, &mut nw, &mut used)
    })?;
    Ok((used, nw))
}
