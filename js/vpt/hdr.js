'use strict';
// Radiance .hdr (RGBE) reader for environment maps — the Node host's twin of vpt_amd/hdr.py (same rules, same bytes; see there).
// readHDR(buffer) -> { data: Uint8Array RGBE [height][width][4] (undecoded), width, height, format: 'rgbe' }; setEnvironmentMap uploads it as
// VPT_ENV_RGBE8 and the device decodes it.  FORMAT must be 32-bit_rle_rgbe when given; EXPOSURE and other header lines are ignored (not
// applied); only '-Y H +X W'; new-style RLE or flat scanlines (flat only when W < 8 or W > 32767); old-style RLE, a zero count or truncated
// data throw.  Row 0 is the file's first scanline, the image's top.

function fail(msg) { throw new Error('HDR: ' + msg); }

function readLine(buf, pos) {
    const end = buf.indexOf(10, pos);
    if (end < 0) { fail('truncated header'); }
    return [Buffer.from(buf.buffer, buf.byteOffset + pos, end - pos).toString('latin1'), end + 1];
}

function readHDR(buffer) {
    const buf = buffer instanceof Uint8Array ? buffer : new Uint8Array(buffer);
    let [line, pos] = readLine(buf, 0);
    if (line !== '#?RADIANCE' && line !== '#?RGBE') { fail('not a Radiance file (no #?RADIANCE / #?RGBE line)'); }
    for (;;) {
        [line, pos] = readLine(buf, pos);
        if (line === '') { break; }
        if (line.startsWith('FORMAT=') && line !== 'FORMAT=32-bit_rle_rgbe') { fail('unsupported format ' + line.slice(7) + ' (only 32-bit_rle_rgbe)'); }
    }
    [line, pos] = readLine(buf, pos);
    const m = /^-Y (\d+) \+X (\d+)$/.exec(line);
    if (!m) { fail('unsupported resolution line ' + JSON.stringify(line) + ' (only -Y H +X W)'); }
    const height = Number(m[1]), width = Number(m[2]);
    if (width < 1 || height < 1) { fail('empty image ' + width + 'x' + height); }
    const out = new Uint8Array(width * height * 4);
    const n = buf.length;
    for (let y = 0; y < height; y++) {
        const row = 4 * width * y;
        if (width >= 8 && width <= 32767 && pos + 4 <= n && buf[pos] === 2 && buf[pos + 1] === 2 && buf[pos + 2] < 128) {
            const w = (buf[pos + 2] << 8) | buf[pos + 3];
            if (w !== width) { fail('scanline ' + y + ' has width ' + w + ', the image ' + width); }
            pos += 4;
            for (let c = 0; c < 4; c++) {
                for (let x = 0; x < width;) {
                    if (pos >= n) { fail('truncated scanline data'); }
                    let count = buf[pos++];
                    if (count > 128) {
                        count -= 128;
                        if (x + count > width) { fail('run overruns the scanline'); }
                        if (pos >= n) { fail('truncated scanline data'); }
                        const v = buf[pos++];
                        for (let k = 0; k < count; k++) { out[row + 4 * (x + k) + c] = v; }
                    } else if (count === 0) {
                        fail('zero run count in a scanline');
                    } else {
                        if (x + count > width) { fail('run overruns the scanline'); }
                        if (pos + count > n) { fail('truncated scanline data'); }
                        for (let k = 0; k < count; k++) { out[row + 4 * (x + k) + c] = buf[pos++]; }
                    }
                    x += count;
                }
            }
            continue;
        }
        if (pos + 4 * width > n) { fail('truncated scanline data'); }
        for (let x = 0; x < width; x++) {
            const p = pos + 4 * x;
            if (buf[p] === 1 && buf[p + 1] === 1 && buf[p + 2] === 1) { fail('old-style run-length scanlines (1 1 1 n) are not supported'); }
        }
        out.set(buf.subarray(pos, pos + 4 * width), row);
        pos += 4 * width;
    }
    return { data: out, width, height, format: 'rgbe' };
}

module.exports = { readHDR };
