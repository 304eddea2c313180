--[[ adcensus_train.lua -- adds the training and dataset entries of the reference's `adcensus` table
(adcensus.cu funcs[], 2061-2096) to the table that adcensus.lua builds, on top of libmcops.so
(include/mc_ops.h):

    Normalize_backward_input                            Normalize2.lua:17
    Margin2                                             Margin2.lua:14
    remove_nonvisible, remove_occluded, remove_white    preprocess_kitti.lua:97-99
    make_dataset2                                       preprocess_kitti.lua:110-112
    subset_dataset                                      main.lua:645

Usage (replaces `require 'libadcensus'` in main.lua:327 and preprocess_kitti.lua):

    adcensus = require 'adcensus_train'    -- with libmcadcensus.so and libmcops.so on the library path

Names, argument order and in-place behaviour are the reference's.  Where the reference writes out of bounds
(make_dataset2 past nnz, subset_dataset outside its table of 200 flags) the library refuses and this file raises.

NOTE: LuaJIT/Torch7 are not available in the build image of this repository, so this file cannot be
executed there; tests/test_ops_host.py checks its ffi.cdef block and ABI constant against include/mc_ops.h,
and the identical C ABI is driven from Python ctypes in tests/.
]]
local ffi = require 'ffi'
local adcensus = require 'adcensus'

ffi.cdef[[
int mc_ops_version(void);
const char *mc_ops_last_error(void);
int mc_normalize_backward_input(const float *grad_output, const float *input, const float *norm, float *grad_input,
                                int N, int C, int H, int W, void *stream);
int mc_margin2(const float *input, float *tmp, float *grad_input, int n_pairs, float margin, int pow, void *stream);
int mc_remove_nonvisible(float *disp, int64_t n, int W, void *stream);
int mc_remove_occluded(float *disp, int64_t n, int W, void *stream);
int mc_remove_white(const float *x, float *disp, int64_t n, void *stream);
int mc_make_dataset2(const float *disp, int H, int W, float *nnz, int64_t nnz_rows, int img, int64_t t, int64_t *t_out);
int mc_subset_dataset(const int64_t *index, int64_t n_index, const float *input, int64_t n_rows, float *output, int64_t *n_out);
]]

local lib = ffi.load('mcops')
local MC_OPS_ABI_VERSION = 1   -- include/mc_ops.h; tests/test_ops_host.py checks this constant and every prototype above
assert(lib.mc_ops_version() == MC_OPS_ABI_VERSION, ('libmcops ABI version %d, this shim is written for %d'):format(
   lib.mc_ops_version(), MC_OPS_ABI_VERSION))

local function check(rc, what)
   if rc ~= 0 then
      error(('%s: %s (rc=%d)'):format(what, ffi.string(lib.mc_ops_last_error()), rc), 3)
   end
end

-- luaT_checkudata(L, i, <type>) + the contiguity the reference silently assumes
local function ptr(t, what, typename)
   typename = typename or 'torch.CudaTensor'
   if torch.typename(t) ~= typename then
      error(('%s: %s expected, got %s'):format(what, typename, torch.typename(t) or type(t)), 3)
   end
   if not t:isContiguous() then
      error(what .. ': contiguous tensor expected', 3)
   end
   return t:data()
end

function adcensus.Normalize_backward_input(grad_output, input, norm, grad_input)   -- adcensus.cu:1359-1377
   local what = 'Normalize_backward_input'
   check(lib.mc_normalize_backward_input(ptr(grad_output, what), ptr(input, what), ptr(norm, what), ptr(grad_input, what),
                                         input:size(1), input:size(2), input:size(3), input:size(4), nil), what)
end

function adcensus.Margin2(input, tmp, gradInput, margin, pow)   -- adcensus.cu:1425-1453
   check(lib.mc_margin2(ptr(input, 'Margin2'), ptr(tmp, 'Margin2'), ptr(gradInput, 'Margin2'), tmp:nElement(), margin, pow, nil),
         'Margin2')
end

function adcensus.remove_nonvisible(y)                       -- adcensus.cu:1734-1745
   check(lib.mc_remove_nonvisible(ptr(y, 'remove_nonvisible'), y:nElement(), y:size(4), nil), 'remove_nonvisible')
end

function adcensus.remove_occluded(y)                         -- adcensus.cu:1761-1772
   check(lib.mc_remove_occluded(ptr(y, 'remove_occluded'), y:nElement(), y:size(4), nil), 'remove_occluded')
end

function adcensus.remove_white(x, y)                         -- adcensus.cu:1784-1796
   if x:nElement() < y:nElement() then
      error(('remove_white: the image holds %d elements, the map %d'):format(x:nElement(), y:nElement()), 2)
   end
   check(lib.mc_remove_white(ptr(x, 'remove_white'), ptr(y, 'remove_white'), y:nElement(), nil), 'remove_white')
end

-- host side (torch.FloatTensor / torch.LongTensor arguments, as in the reference)
function adcensus.make_dataset2(disp, nnz, img, t)           -- adcensus.cu:1900-1929
   local t_out = ffi.new('int64_t[1]')
   check(lib.mc_make_dataset2(ptr(disp, 'make_dataset2', 'torch.FloatTensor'), disp:size(3), disp:size(4),
                              ptr(nnz, 'make_dataset2', 'torch.FloatTensor'), math.floor(nnz:nElement() / 4), img, t, t_out),
         'make_dataset2')
   return tonumber(t_out[0])
end

function adcensus.subset_dataset(index, input, output)       -- adcensus.cu:1863-1898
   if output:nElement() < input:nElement() then
      error(('subset_dataset: the output holds %d elements, the input %d'):format(output:nElement(), input:nElement()), 2)
   end
   local n_out = ffi.new('int64_t[1]')
   check(lib.mc_subset_dataset(ptr(index, 'subset_dataset', 'torch.LongTensor'), index:nElement(),
                               ptr(input, 'subset_dataset', 'torch.FloatTensor'), input:size(1),
                               ptr(output, 'subset_dataset', 'torch.FloatTensor'), n_out), 'subset_dataset')
   return tonumber(n_out[0])
end

return adcensus
